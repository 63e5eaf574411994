"""CPU-only: the numpy restatement of ``GenerateClampedTrajectory`` (tests/clamp_ref.py) against what the TRUE reference
returned (tests/golden/clamped_known_answers.npz, made by tools/make_clamp_goldens.py) - bit for bit, there is no
tolerance: every value is a copy or a fixed sequence of IEEE operations - and the equivalences that carry those goldens,
which exist for all-mobile structures only, over to structures with static atoms."""
import numpy as np
import pytest

from tests import clamp_ref as CR

CG = CR.ClampGoldens()


def test_recorded_errors_of_the_reference():
    z = CG.z
    assert str(z["static_atom_error"]) == "IndexError"           # the reference does not run on a real structure
    assert str(z["empty_mask_error"]) == "ValueError"
    assert str(z["unassigned_error"]) == "RuntimeError"
    assert str(z["partial_no_real_error"]) == "RuntimeError"
    assert CG.names == ["triclinic_big", "triclinic_one", "ortho_big", "ortho_one"]


@pytest.mark.parametrize("name", CG.names)
def test_margins_of_the_goldens(name):
    i = CG.inputs(name)
    m_img, m_floor = CR.margins(i["cell"], i["centers"], i["labels"], i["positions"])
    assert m_img == float(CG.z[name + "/margin_image"]) and m_floor == float(CG.z[name + "/margin_floor"])
    assert m_img >= CR.MARGIN and m_floor >= CR.MARGIN
    # what the fixture was asked to cover
    crystal_centers = CR.to_cell(i["cell"], i["centers"])
    crystal_pos = CR.to_cell(i["cell"], i["positions"])
    assert crystal_centers.min() >= -0.5 - 1e-9 and crystal_centers.max() <= 1.5 + 1e-9
    if len(i["labels"]) > 1:
        assert crystal_centers.min() < 0 and crystal_centers.max() > 1
        assert crystal_pos.min() < -2 and crystal_pos.max() > 3
        un = i["labels_unassigned"]
        assert np.all(un[:, 3] == -1) and un[0, 0] == un[-1, 0] == -1 and un[17, 1] == -1 and np.sum(un[:, 1] == -1) == 1
    assert not np.any(i["labels"] == -1)


@pytest.mark.parametrize("name", CG.names)
def test_restatement_reproduces_the_reference(name):
    i = CG.inputs(name)
    M = i["labels"].shape[1]
    outs = CG.outputs(name)
    assert len(outs) == 4 + 2 + 2                                # unassigned labels without pass-through: the reference raises
    for key, w, p, mask, with_real, expected in outs:
        got = CR.clamp(i["cell"], i["ref_positions"], np.ones(M, dtype=bool), i["centers"], i[key],
                       i["positions"] if with_real else None, mask, w, p)
        assert got.dtype == np.float64 and np.array_equal(got, expected), (key, w, p)
        if w and key == "labels":
            assert np.array_equal(expected, i["centers"][i[key]])
    for w in (False, True):
        with pytest.raises(RuntimeError):
            CR.clamp(i["cell"], i["ref_positions"], np.ones(M, dtype=bool), i["centers"], i["labels_unassigned"],
                     i["positions"], None, w, False)


def test_unwrapped_centre_goes_into_the_output():
    """The search sees the WRAPPED centre, the output is built on the crystal coordinates of the centre as given: for a
    centre outside the cell the result is an image of the centre, and not always the one nearest the position."""
    i = CG.inputs("triclinic_big")
    out = CG.z["triclinic_big/out_labels_w0p0"]
    shift = CR.to_cell(i["cell"], out) - CR.to_cell(i["cell"], i["centers"])[i["labels"]]
    assert np.max(np.abs(shift - np.round(shift))) < 1e-12       # a lattice vector away from the centre as given
    wrapped, _ = CR.wrap(i["cell"], i["centers"])
    w, _ = CR.wrap(i["cell"], i["positions"])
    d = CR.image_distances(i["cell"], w, wrapped[i["labels"]])
    assert np.any(np.linalg.norm(out - i["positions"], axis=-1) > d.min(axis=-1) + 1e-6)


@pytest.mark.parametrize("layout", ["first", "last", "interleaved"])
@pytest.mark.parametrize("wrap,pass_through", CR.COMBOS)
def test_static_atoms_in_any_order(layout, wrap, pass_through):
    """With static atoms anywhere in the structure: the clamped mobile columns are the all-mobile operator's on the
    mobile sub-structure, clamped static atoms stand on the structure's positions, unclamped atoms keep theirs."""
    F, M, K = 9, 4, 3
    centers, labels, pos = CR.designed(CR.TRICLINIC, F, M, K, seed=5, n_unknown=3 if pass_through else 0)
    mobile, spos = CR.structure(M, 5, layout, seed=3)
    real = CR.embed(mobile, spos, pos, seed=4)
    sub = CR.clamp_mobile(CR.TRICLINIC, centers, labels, pos, wrap, pass_through)
    full = CR.clamp(CR.TRICLINIC, spos, mobile, centers, labels, real, None, wrap, pass_through)
    assert np.array_equal(full[:, mobile], sub)
    assert np.array_equal(full[:, ~mobile], np.broadcast_to(spos[~mobile], (F,) + spos[~mobile].shape))
    mask = np.random.default_rng(8).uniform(size=len(mobile)) < 0.5
    part = CR.clamp(CR.TRICLINIC, spos, mobile, centers, labels, real, mask, wrap, pass_through)
    assert np.array_equal(part[:, ~mask], real[:, ~mask])
    assert np.array_equal(part[:, mask], full[:, mask])
