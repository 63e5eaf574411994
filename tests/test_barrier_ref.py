"""CPU-only: the numpy restatement of ``MergeSitesByBarrier`` (tests/barrier_ref.py) reproduces every case of the TRUE
reference's goldens (tests/golden/barrier_known_answers.npz, tools/make_barrier_goldens.py) exactly: the error, the mergable
matrix, the groups, the merged trajectory, centres and site types.  The GPU tests compare the device against this restatement
on inputs the goldens do not hold, so it is pinned here first."""
import json

import numpy as np
import pytest

from tests import barrier_ref as BR

BG = BR.BarrierGoldens()


def test_the_golden_inputs_are_the_designed_cases():
    cases = BR.golden_case_inputs()
    assert BG.names == list(cases)
    for name, case in cases.items():
        stored = BG.case(name)
        for k in BR.INPUT_KEYS + ["site_types", "coordinating_mask"]:
            assert (stored[k] is None and case[k] is None) or np.array_equal(stored[k], case[k]), (name, k)
        assert stored["lj"] == case["lj"] and stored["kw"] == case["kw"]


@pytest.mark.parametrize("name", BG.names)
def test_restatement_equals_the_reference(name):
    case, exp = BG.case(name), BG.expected(name)
    got = BR.run_case(case)
    assert got["error"] == exp["error"]
    assert got["mergable"].dtype == np.bool_ and np.array_equal(got["mergable"], exp["mergable"])
    assert len(got["groups"]) == len(exp["groups"]) and all(np.array_equal(a, b) for a, b in zip(got["groups"], exp["groups"]))
    assert np.array_equal(got["pairs"], exp["pairs"])
    assert got["energies"].tobytes() == exp["energies"].tobytes()
    if not exp["error"]:
        assert np.array_equal(got["traj"], exp["traj"])
        assert np.array_equal(got["centers"], exp["centers"])
        if case["kw"].get("check_types"):
            assert np.array_equal(got["site_types"], exp["site_types"])
    else:
        assert "traj" not in exp


@pytest.mark.parametrize("name", BG.names)
def test_no_golden_decision_hinges_on_the_last_bit(name):
    """Every barrier stays MARGIN x max |E| from the threshold and every maximum from the ends, and the reference's totals
    (the lattice's own energy included) are the mobile atom's energies up to their rounding."""
    case, exp = BG.case(name), BG.expected(name)
    assert float(BG.z["margin"]) == BR.MARGIN
    if len(exp["pairs"]):
        assert (exp["margins"] >= BR.MARGIN).all()
        recomputed = np.array([BR.margins(row, case["kw"]["barrier_threshold"]) for row in exp["energies"]])
        assert np.array_equal(recomputed, exp["margins"])
        shift = exp["totals"] - exp["energies"]
        assert np.ptp(shift) <= 1e-12 * max(1.0, np.abs(exp["totals"]).max())
        assert exp["n_terms"].max() <= 100000


def test_every_kind_of_case_is_there():
    kinds = json.loads(str(BG.z["kinds"]))
    assert sorted(kinds) == sorted(BR.KINDS) and all(kinds[k] for k in BR.KINDS)
    assert str(BG.z["no_n_ij_error"]) == "NameError"
