"""No GPU: the inputs of tests/test_gpu_dynamic_mapping.py are what they claim to be.  For every case the oracle with
dynamic lattice mapping on the permuted frames gives, bit for bit, the rows of the oracle without mapping on the unpermuted
frames (so no argmin went to a neighbour and the two references of the GPU tests are one), and the permuted frames without
mapping raise StaticLatticeError (so the inputs do need the map)."""
import numpy as np
import pytest

from tests import dynmap_ref as R

INPUTS = sorted(set((cfg, M, F, mode, False) for cfg, M, F, mode, _ in R.ROW_CASES)
                | set((cfg, M, F, mode, False) for cfg, M, F, mode in R.OPERATOR_CASES)
                | {("C2", 64, 12, "mixed", True), ("C2", 64, 12, "all", True)})


def _first_permuted_frame(perms):
    return int(np.flatnonzero((perms != np.arange(perms.shape[1])).any(axis=1))[0])


@pytest.mark.parametrize("mode", ["all", "mixed", "rotate"])
def test_permute_statics_moves_only_the_static_atoms(mode):
    rng = np.random.default_rng(3)
    frames = rng.normal(size=(7, 25, 3))
    sidx = np.sort(rng.choice(25, size=20, replace=False))
    pf, perms = R.permute_statics(frames, sidx, 5, mode)
    rest = np.setdiff1d(np.arange(25), sidx)
    assert np.array_equal(pf[:, rest], frames[:, rest])
    for f in range(7):
        assert np.array_equal(np.sort(perms[f]), np.arange(20))
        assert np.array_equal(pf[f, sidx], frames[f, sidx[perms[f]]])
    ident = (perms == np.arange(20)).all(axis=1)
    if mode == "mixed":
        assert np.array_equal(np.flatnonzero(ident), [0, 3, 6])
    else:
        assert not ident.any()
    if mode == "rotate":
        assert np.array_equal(perms[2], np.roll(np.arange(20), 3))
    assert any(not np.array_equal(perms[f], perms[f + 1]) for f in range(6))


@pytest.mark.parametrize("cfg,M,F,mode,shove", INPUTS)
def test_mapping_undoes_the_permutation_bit_for_bit(oracle, cfg, M, F, mode, shove):
    c = R.case(cfg, M, F, mode, shove)
    (mapped, nz_mapped), (plain, nz_plain) = R.references(cfg, M, F, mode, shove)
    assert nz_mapped == nz_plain
    assert np.array_equal(mapped, plain)
    assert (mapped != 0).any()
    with pytest.raises(oracle.OracleError) as ei:
        R.oracle_fill(c, c.pf)
    assert ei.value.kind == "StaticLatticeError" and ei.value.frame == _first_permuted_frame(c.perms)


def test_split_case_has_two_frames_beyond_delta_and_none_near_it(oracle):
    """The "mixed" input of the tight / loose test: the displacement sample keeps the unpermuted frames 0, 3, 6, 9; the
    two shoved frames (2 and 7) and only they lie beyond the bound it gives, none within 1e-6 of it.  The "all" input:
    every sample is thrown away, the bound is the floor and every frame lies beyond it."""
    c = R.case("C2", 64, 12, "mixed", True)
    assert all(s >= 256 for _, s, _ in R.SPLIT_SHOVES)
    dm = R.matched_dmax(oracle, c.cell, c.ref_static, c.frames, c.sidx)
    own = R.matched_dmax(oracle, c.cell, c.ref_static, c.pf, c.sidx)
    assert dm.max() < 1.0
    assert np.array_equal(np.flatnonzero(own <= 1.0), [0, 3, 6, 9])
    delta = R.expected_delta(own)
    assert np.array_equal(np.flatnonzero(dm > delta), [2, 7])
    assert np.abs(dm - delta).min() > 1e-6
    c = R.case("C2", 64, 12, "all", True)
    own = R.matched_dmax(oracle, c.cell, c.ref_static, c.pf, c.sidx)
    assert R.expected_delta(own) == 0.02 and (dm > 0.02 + 1e-6).all()


@pytest.mark.parametrize("cfg,M,F", R.ERROR_CASES)
def test_error_inputs_and_the_order_the_reference_reports_them_in(oracle, cfg, M, F):
    c, pf, perms = R.threshold_case(cfg, M, F)
    assert c.S > 256
    with pytest.raises(oracle.OracleError) as ei:
        R.oracle_fill(c, pf, dynamic_lattice_mapping=True)
    assert (ei.value.kind, ei.value.frame, list(ei.value.lattice_atoms)) == ("StaticLatticeError", 3, [c.S - 4])
    c, pf, perms, a = R.unassigned_case(cfg, M, F)
    assert min(R.unassigned_sites(c.S)) >= 256
    with pytest.raises(oracle.OracleError) as ei:
        R.oracle_fill(c, pf, dynamic_lattice_mapping=True, static_movement_threshold=5.0)
    assert ei.value.kind == "StaticLatticeError" and ei.value.frame == 4
    assert np.array_equal(ei.value.lattice_atoms, np.flatnonzero(perms[4] == a))     # indices in the permuted order
    rows, _ = R.oracle_fill(c, pf, dynamic_lattice_mapping=True, static_movement_threshold=5.0, relaxed_lattice_checks=True)
    assert (rows != 0).any()
    with pytest.raises(oracle.OracleError) as ei:                                    # both kinds in frame 4: the threshold first
        R.oracle_fill(c, pf, dynamic_lattice_mapping=True)
    assert (ei.value.kind, ei.value.frame, list(ei.value.lattice_atoms)) == ("StaticLatticeError", 4, [a])
