"""GPU: dynamic lattice mapping with maps that are NOT the identity, through the C-ABI.

``dynamic_lattice_mapping=True`` is the one mode in which the fill kernels read every static atom through the per-frame
table that ``k_lattice_map`` builds; a synthetic trajectory never reorders its static atoms, so everywhere else in the
suite that table is ``arange(S)`` in every frame.  Here the static atoms of every frame are permuted, with another
permutation per frame (tests/dynmap_ref.py).  The reference's mapping undoes the permutation, which gives two references
that are not the code under test and that agree bit for bit (tests/test_dynmap_ref.py, asserted again here): the oracle
with mapping on the permuted frames, the oracle without mapping on the unpermuted ones.  A kernel that ignored the map,
read it with the wrong frame or with the wrong stride fails these tests."""
import contextlib

import numpy as np
import pytest

from tests import dynmap_ref as R

pytestmark = pytest.mark.gpu

KNOBS = ("SITATOR_FILL_WAVES", "SITATOR_FILL_FPB", "SITATOR_FILL_RCAP", "SITATOR_FILL_IW", "SITATOR_FILL_CONTIG",
         "SITATOR_FILL_TCAP")


@pytest.fixture
def make_ctx(monkeypatch):
    """Contexts on the basis of a case, closed when the test ends - also when it fails."""
    from sitator_amd import _lib
    made = []

    def make(c, frames, kernel=3, static_thr=1.0, frame0=0):
        with monkeypatch.context() as mp:
            mp.setenv("SITATOR_FILL_KERNEL", str(kernel))
            ctx = _lib.HipContext(c.cell)
            made.append(ctx)
            ctx.set_basis(c.ref_static, c.verts, c.vcd, 1.5, 30, static_thr)
        ctx.set_frames(frames, c.sidx, c.midx, frame0=frame0)
        return ctx

    yield make
    for ctx in made:
        ctx.close()


def _fill(ctx, monkeypatch=None, env=None, **kw):
    """Rows and zero count of one fill with mapping; ``env``: knobs that hold for this fill alone."""
    with (monkeypatch.context() if env else contextlib.nullcontext()) as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        rc, nz, err = ctx.fill(dynamic_lattice_mapping=True, check_for_zeros=False, **kw)
    assert rc == 0, (rc, err.frame, err.index)
    return ctx.rows_dense(), nz


def _assert_oracle_rows(got, nz, exp, nz_exp):
    assert nz == nz_exp
    assert np.array_equal(got != 0, exp != 0)
    np.testing.assert_allclose(got, exp, rtol=1e-12, atol=0)


def _oracle_error(oracle, c, pf, **kw):
    with pytest.raises(oracle.OracleError) as ei:
        R.oracle_fill(c, pf, dynamic_lattice_mapping=True, **kw)
    assert ei.value.kind == "StaticLatticeError"
    return ei.value


# ---- 1. rows under a non-identity map ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg,M,F,mode,kernel", R.ROW_CASES)
def test_rows_under_a_non_identity_map(make_ctx, cfg, M, F, mode, kernel):
    """Rows of the permuted frames with mapping against both oracle references: the same zero count, the same zero
    pattern, values within 1e-12 (the bar of test_third_generation_rows_match_oracle).  k_fill3 also fills the UNPERMUTED
    frames with mapping in the same context: those rows are the permuted frames' rows BIT FOR BIT (array_equal, not a
    tolerance) - the same coordinates go through the same arithmetic wherever the atom sits in the frame, and the tight and
    the loose table differ in what they prune, not in what they compute.  The hosts with four ions (C1d, C1b) run several
    frames per workgroup by themselves."""
    c = R.case(cfg, M, F, mode)
    (exp, nz_exp), (plain, nz_plain) = R.references(cfg, M, F, mode)
    assert nz_exp == nz_plain and np.array_equal(exp, plain), "the two references must be one"
    ctx = make_ctx(c, c.pf, kernel)
    got, nz = _fill(ctx)
    assert ctx.info()["fill_kernel"] == kernel, "the requested kernel generation did not run"
    if M == 4:
        assert ctx.info()["frames_per_workgroup"] > 1
    _assert_oracle_rows(got, nz, exp, nz_exp)
    if kernel == 3:
        ctx.set_frames(c.frames, c.sidx, c.midx)
        same, nz_same = _fill(ctx)
        assert ctx.info()["fill_kernel"] == 3
        _assert_oracle_rows(same, nz_same, exp, nz_exp)
        assert nz_same == nz and np.array_equal(got, same)


# ---- 2. the three places where k_fill3 reads the map, forced -------------------------------------------------------------------

# waves, frames per workgroup, survivor slots, ions per window, copy mode, task table, frames
SHAPES = [("4", "1", "48", "16", "2", "128", 12),       # the single-frame set-up
          ("4", "3", "64", "64", "0", "512", 12),       # the multi-frame set-up, every workgroup full
          ("4", "4", "16", "33", "2", "256", 10),       # a ragged last workgroup (frames 8 and 9)
          ("4", "2", "8", "5", "1", "64", 12),          # few survivor slots, a small task table: several rounds per window
          ("8", "1", "8", "16", "1", "64", 12)]         # the same in the single-frame form


@pytest.mark.parametrize("waves,fpb,rcap,iw,contig,tcap,F", SHAPES)
def test_launch_shapes_agree_under_a_non_identity_map(make_ctx, monkeypatch, waves, fpb, rcap, iw, contig, tcap, F):
    """C2 with the statics rotated by f + 1 places in frame f (a wrong frame index reads an atom that is in range but
    wrong).  However the work is cut up - one frame per workgroup or several, a ragged last workgroup, so few survivor
    slots and task-table entries that a window takes several rounds - the rows are those of the default launch shape bit
    for bit (test_third_generation_launch_shapes_agree asserts this without mapping), and the context says that the shape
    asked for was the shape taken."""
    c = R.case("C2", 64, 12, "rotate")
    (exp, nz_exp), _ = R.references("C2", 64, 12, "rotate")
    ctx = make_ctx(c, c.pf[:F])
    base, nz_base = _fill(ctx)
    assert ctx.info()["fill_kernel"] == 3
    exp = exp[:F * 64]
    _assert_oracle_rows(base, nz_base, exp, int(np.count_nonzero(~(exp != 0).any(axis=1))))
    env = dict(zip(KNOBS, (waves, fpb, rcap, iw, contig, tcap)))
    got, nz = _fill(ctx, monkeypatch, env)
    info = ctx.info()
    assert info["fill_kernel"] == 3
    assert info["waves_per_workgroup"] == int(waves) and info["frames_per_workgroup"] == int(fpb)
    assert info["survivors_per_wave"] == int(rcap) and info["task_table_per_wave"] == int(tcap)
    assert nz == nz_base and np.array_equal(base, got)


@pytest.mark.parametrize("fpb", ["1", "3"])
def test_exact_and_general_cell_arithmetic_agree_under_a_non_identity_map(make_ctx, monkeypatch, fpb):
    """SITATOR_F3_FORCE_EXACT=1 (every pass goes round again with the reference's arithmetic) and SITATOR_F3_CHEAP=0 (the
    general-cell instantiation on the diagonal cell), in the single-frame and in the multi-frame set-up: the same zero
    pattern, values within 1e-13 (as test_cheap_distance_and_reference_distance_agree), every one against the oracle."""
    c = R.case("C2", 64, 12, "rotate")
    (exp, nz_exp), _ = R.references("C2", 64, 12, "rotate")
    ctx = make_ctx(c, c.pf)
    monkeypatch.setenv("SITATOR_FILL_WAVES", "4")
    monkeypatch.setenv("SITATOR_FILL_FPB", fpb)
    out = []
    for env in ({}, {"SITATOR_F3_FORCE_EXACT": "1"}, {"SITATOR_F3_CHEAP": "0"}):
        rows, nz = _fill(ctx, monkeypatch, env)
        info = ctx.info()
        assert info["fill_kernel"] == 3 and info["frames_per_workgroup"] == int(fpb)
        if "SITATOR_F3_FORCE_EXACT" in env:
            assert info["band_redos"] > 0, "the band was not forced open"
        _assert_oracle_rows(rows, nz, exp, nz_exp)
        out.append((rows, nz))
    for rows, nz in out[1:]:
        assert nz == out[0][1]
        assert np.array_equal(out[0][0] != 0, rows != 0)
        np.testing.assert_allclose(rows, out[0][0], rtol=1e-13, atol=0)


# ---- 3. the tight / loose split under mapping -------------------------------------------------------------------------------

def test_frames_beyond_delta_take_the_loose_table_under_mapping(make_ctx, oracle):
    """Under mapping k_fill3 takes a frame's tight / loose decision from frame_dmax, the matched distances that
    k_lattice_map wrote.  Two frames (2 and 7) have one static atom - lattice sites 300 and 411, beyond the first 256 -
    shoved by 0.6 A, below static_movement_threshold; the statics are permuted in two frames of three.  The displacement
    sample keeps the unpermuted frames only, delta follows from them, and exactly the two shoved frames lie beyond it
    (none within 1e-6 of it, so the squared comparison is not in doubt); rows against the oracle."""
    c = R.case("C2", 64, 12, "mixed", True)
    (exp, nz_exp), (plain, nz_plain) = R.references("C2", 64, 12, "mixed", True)
    assert nz_exp == nz_plain and np.array_equal(exp, plain)
    dm = R.matched_dmax(oracle, c.cell, c.ref_static, c.frames, c.sidx)
    ctx = make_ctx(c, c.pf)
    got, nz = _fill(ctx)
    info = ctx.info()
    assert info["fill_kernel"] == 3
    _assert_oracle_rows(got, nz, exp, nz_exp)
    delta = info["delta"]
    assert np.abs(dm - delta).min() > 1e-6
    assert info["fallback_frames"] == np.count_nonzero(dm > delta)
    assert np.count_nonzero(dm > delta) == 2


def test_no_valid_displacement_sample_gives_the_floor_and_every_frame_loose(make_ctx, oracle):
    """A fresh permutation in every frame: k_sample_dmax measures own-index distances, every one of them is beyond the
    threshold and thrown away, delta is the floor (0.02 A), every frame lies beyond it and takes the loose table; rows
    against the oracle."""
    c = R.case("C2", 64, 12, "all", True)
    (exp, nz_exp), (plain, nz_plain) = R.references("C2", 64, 12, "all", True)
    assert nz_exp == nz_plain and np.array_equal(exp, plain)
    ctx = make_ctx(c, c.pf)
    got, nz = _fill(ctx)
    info = ctx.info()
    assert info["fill_kernel"] == 3
    assert info["delta"] == 0.02
    assert info["delta"] >= 0 and info["fallback_frames"] == c.F
    _assert_oracle_rows(got, nz, exp, nz_exp)


# ---- 4. the error contract of k_lattice_map at S > 256 ----------------------------------------------------------------------

@pytest.mark.parametrize("cfg,M,F", R.ERROR_CASES)
def test_threshold_error_is_the_first_in_the_reference_order(make_ctx, oracle, cfg, M, F):
    """Frame 3: the atoms of lattice sites S - 3 and S - 4 (beyond the first 256) are further than the threshold from
    every lattice position; frame 6: the atom of site 1.  The reference stops at the earliest frame and, in it, at the
    lowest lattice site: (3, S - 4), whatever the order of the atoms in the frame; frame numbers count from frame0."""
    from sitator_amd import _lib
    c, pf, perms = R.threshold_case(cfg, M, F)
    e = _oracle_error(oracle, c, pf)
    assert (e.frame, list(e.lattice_atoms)) == (3, [c.S - 4])
    for frame0 in (0, 1000):
        ctx = make_ctx(c, pf, frame0=frame0)
        rc, nz, err = ctx.fill(dynamic_lattice_mapping=True, check_for_zeros=False)
        assert rc == _lib.E_STATIC_THRESHOLD
        assert (err.frame, err.index) == (frame0 + e.frame, e.lattice_atoms[0]) == (frame0 + 3, c.S - 4)


@pytest.mark.parametrize("cfg,M,F", R.ERROR_CASES)
def test_unassigned_atom_and_which_kind_wins(make_ctx, oracle, cfg, M, F):
    """Frame 4: static atom a sits 0.3 A beside atom b (lattice sites beyond the first 256), so no lattice position has
    a as its nearest atom.  With a loose threshold: E_STATIC_UNASSIGNED at frame 4, and the atoms nobody saw are the
    oracle's - indices in the order of the (permuted) frame; with relaxed_lattice_checks the fill runs and the rows are the
    oracle's.  With the default threshold lattice site a is a threshold error in the same frame, and that is what the
    reference reports."""
    from sitator_amd import _lib
    c, pf, perms, a = R.unassigned_case(cfg, M, F)
    e = _oracle_error(oracle, c, pf, static_movement_threshold=5.0)
    assert e.frame == 4 and len(e.lattice_atoms) == 1 and perms[4][e.lattice_atoms[0]] == a
    ctx = make_ctx(c, pf, static_thr=5.0)
    rc, nz, err = ctx.fill(dynamic_lattice_mapping=True, check_for_zeros=False)
    assert rc == _lib.E_STATIC_UNASSIGNED and err.frame == e.frame
    assert np.array_equal(np.flatnonzero(ctx.static_seen(4) == 0), e.lattice_atoms)
    exp, nz_exp = R.oracle_fill(c, pf, dynamic_lattice_mapping=True, static_movement_threshold=5.0,
                                relaxed_lattice_checks=True)
    got, nz = _fill(ctx, relaxed_lattice_checks=True)
    _assert_oracle_rows(got, nz, exp, nz_exp)
    e = _oracle_error(oracle, c, pf)                            # both kinds in frame 4
    assert (e.frame, list(e.lattice_atoms)) == (4, [a])
    ctx = make_ctx(c, pf)
    rc, nz, err = ctx.fill(dynamic_lattice_mapping=True, check_for_zeros=False)
    assert rc == _lib.E_STATIC_THRESHOLD and (err.frame, err.index) == (e.frame, e.lattice_atoms[0])


# ---- 5. the operator ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg,M,F,mode", R.OPERATOR_CASES)
def test_operator_with_mapping_on_permuted_frames(oracle, cfg, M, F, mode):
    """LandmarkAnalysis(dynamic_lattice_mapping=True) on the permuted frames: the labels of the oracle's operator on the
    same frames and of LandmarkAnalysis() on the unpermuted ones, bit for bit; confidences and site centres within the bar
    of the end-to-end fuzz."""
    from sitator_amd import LandmarkAnalysis, SiteNetwork, Structure
    c = R.case(cfg, M, F, mode)

    def run(frames, **opts):
        sn = SiteNetwork(Structure(c.ref, c.cell), c.sm, c.mm)
        sn.centers = c.host.centers
        sn.vertices = c.host.vertices
        st = LandmarkAnalysis(verbose=False, **opts).run(sn, np.array(frames))
        return st.traj.copy(), st.confidences.copy(), np.asarray(st.site_network.centers).copy()

    exp = oracle.landmark_analysis(c.cell, c.ref, c.sm, c.mm, c.host.centers, c.host.vertices, c.pf,
                                   dynamic_lattice_mapping=True)
    lab, conf, cen = run(c.pf, dynamic_lattice_mapping=True)
    lab_u, conf_u, cen_u = run(c.frames)
    assert np.array_equal(lab, exp["labels"])
    assert np.array_equal(lab, lab_u)
    assert (lab >= 0).any()
    m = lab >= 0
    for other_conf, other_cen in ((exp["confs"], exp["site_centers"]), (conf_u, cen_u)):
        np.testing.assert_allclose(conf[m], other_conf[m], rtol=1e-6)
        np.testing.assert_allclose(cen, other_cen, rtol=1e-6, atol=1e-9)
