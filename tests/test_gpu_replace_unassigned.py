"""GPU: the two-directional label scan of dynamics.hip (``k_label_chunk_summary``, ``k_rup_*``, ``k_rc_*``) behind ``sit_label_ends``,
``sit_replace_unassigned``, ``sit_unknown_runs`` and ``sit_replace_closer``, and ``ReplaceUnassignedPositions`` on top of
them - against the reference's goldens (tests/golden/replace_unassigned_known_answers.npz) and against the numpy brute
force of tests/replace_ref.py on designed and hand-built label sets.

The kernels cut the frames into chunks of ``CHUNK``, put the ions across lanes in groups of 64 and chain per-(chunk, ion)
summaries forwards and backwards.  What that can get wrong is planted below: runs that begin or end on a chunk's first or
last frame, a run that covers a chunk exactly, a run over three chunks, ions that are never known, M above 64 and above
128, M = 1, a ragged last chunk, one frame, no frame."""
import numpy as np
import pytest

from tests import replace_ref as R

pytestmark = pytest.mark.gpu

CHUNK = 256                                          # LS_CHUNK of label_scan.h
RG = R.ReplaceGoldens()
K = R.K_DESIGNED


class Device(object):
    """A context holding ``labels`` (closed on exit)."""

    def __init__(self, labels, frame0=0, cell=R.CELL):
        self.labels, self.frame0, self.cell = np.asarray(labels, dtype=np.int64), frame0, cell

    def __enter__(self):
        from sitator_amd import _lib
        self.ctx = _lib.HipContext(self.cell)
        self.ctx.set_assignments(self.labels, frame0=self.frame0)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()


def check_against_brute_force(oracle, lab, centers, pos, before_in=None, after_in=None, frame0=0):
    """All four device calls on ``lab`` against the brute force, bit for bit; returns the records."""
    exp_closer, margin = R.closer(oracle, R.CELL, lab, centers, pos, before_in, after_in)
    assert margin >= R.MARGIN                                  # no decided frame is a near-tie (checked on the CPU)
    exp_rec, exp_npos = R.runs(lab, before_in, after_in, frame0)
    with Device(lab, frame0) as ctx:
        version = ctx.labels_version
        first, last = ctx.label_ends()
        assert np.array_equal(first, R.ends(lab)[0]) and np.array_equal(last, R.ends(lab)[1])
        for mode in (0, 1):
            got = ctx.replace_unassigned(mode, before_in, after_in)
            assert got.dtype == np.int64 and np.array_equal(got, R.replace(lab, mode, before_in, after_in)), mode
        rec, npos = ctx.unknown_runs(before_in, after_in)
        assert rec.shape == exp_rec.shape and np.array_equal(rec, exp_rec) and npos == exp_npos
        rec2, npos2 = ctx.unknown_runs(before_in, after_in)
        assert np.array_equal(rec, rec2) and npos == npos2      # the same order on every call
        positions = R.positions_of(rec, pos, frame0)
        assert positions.shape == (npos, 3)
        got = ctx.replace_closer(rec, centers, positions)
        assert np.array_equal(got, exp_closer)
        # the resident labels were only read
        assert ctx.labels_version == version
        assert np.array_equal(ctx.assignments()[0].reshape(lab.shape), lab)
    return rec


# ---- 1. the reference's goldens through the real context ------------------------------------------------------------

@pytest.mark.parametrize("name", RG.names)
def test_gpu_operator_matches_the_reference(oracle, name):
    R.check_golden_case(RG, name, margin_oracle=oracle)


# ---- 2. designed labels against brute force -------------------------------------------------------------------------

@pytest.mark.parametrize("F,M", [(131, 70), (259, 5), (67, 130), (513, 1), (256, 3), (257, 65)])
@pytest.mark.parametrize("halo", [False, True], ids=["no_halo", "halo"])
def test_designed_labels_bit_equal_to_brute_force(oracle, F, M, halo):
    lab = R.designed_labels(F, M, seed=3)
    centers, pos = R.designed_geometry(F, M, seed=3)
    unknown = (lab == -1).mean()
    print("F=%d M=%d: %.1f%% unknown" % (F, M, 100.0 * unknown))
    assert 0.3 < unknown < 0.7
    before_in, after_in = R.halos(M, seed=3) if halo else (None, None)
    rec = check_against_brute_force(oracle, lab, centers, pos, before_in, after_in, frame0=1000 if halo else 0)
    assert len(rec) >= M and (rec[:, 5] >= 0).any() and (rec[:, 5] < 0).any()
    if halo:
        assert rec[:, 1].min() >= 1000 and rec[:, 2].max() <= 1000 + F


def test_a_small_record_buffer_returns_the_count_and_writes_nothing():
    import ctypes as C
    from sitator_amd import _lib
    lab = R.designed_labels(131, 70, seed=3)
    exp, exp_npos = R.runs(lab)
    with Device(lab) as ctx:
        buf = np.full((5, 6), 77, dtype=np.int64)
        n, npos = C.c_int64(0), C.c_int64(0)
        ctx._check(ctx.lib.sit_unknown_runs(ctx._h, None, None, 5, _lib._i(buf), C.byref(n), C.byref(npos)))
        assert n.value == len(exp) > 5 and npos.value == exp_npos and (buf == 77).all()


# ---- 3. hand-built cases --------------------------------------------------------------------------------------------

def _base(F, M=2):
    """Every ion on site (j % K) all along: no run anywhere."""
    return np.tile(np.arange(M) % K, (F, 1)).astype(np.int64)


def _an_ion_never_assigned():
    lab = _base(300, 3)
    lab[:, 1] = -1
    return lab, [(1, 0, 300, -1, -1, -1)]


def _nobody_assigned():
    return np.full((CHUNK + 3, 5), -1, dtype=np.int64), [(j, 0, CHUNK + 3, -1, -1, -1) for j in range(5)]


def _a_run_from_frame_0():
    lab = _base(20)
    lab[:7, 0] = -1
    return lab, [(0, 0, 7, -1, 0, -1)]


def _a_run_to_the_last_frame():
    lab = _base(CHUNK + 20)
    lab[CHUNK - 2:, 1] = -1
    return lab, [(1, CHUNK - 2, CHUNK + 20, 1, -1, -1)]


def _a_run_covering_one_chunk_exactly():
    lab = _base(3 * CHUNK)
    lab[CHUNK:2 * CHUNK, 0] = -1
    lab[2 * CHUNK:, 0] = 4
    return lab, [(0, CHUNK, 2 * CHUNK, 0, 4, 0)]


def _runs_ending_and_starting_on_the_chunk_cut():
    """Ion 0: a run whose last frame is 255; ion 1: a run whose first frame is 256; ion 2: both, frame 255 / 256 apart
    (two runs of one frame would be one run: a known frame 256 stands between 255 and 257)."""
    lab = _base(2 * CHUNK + 1, 3)
    lab[250:CHUNK, 0] = -1
    lab[CHUNK, 0] = 3
    lab[CHUNK:CHUNK + 9, 1] = -1
    lab[CHUNK + 9:, 1] = 5
    lab[CHUNK - 1, 2], lab[CHUNK + 1, 2] = -1, -1
    lab[CHUNK + 2:, 2] = 6
    return lab, [(0, 250, CHUNK, 0, 3, 0), (1, CHUNK, CHUNK + 9, 1, 5, 6), (2, CHUNK - 1, CHUNK, 2, 2, -1),
                 (2, CHUNK + 1, CHUNK + 2, 2, 6, 15)]


def _a_run_across_three_chunks():
    lab = _base(3 * CHUNK + 40)
    lab[CHUNK - 6:2 * CHUNK + 11, 1] = -1
    lab[2 * CHUNK + 11:, 1] = 2
    return lab, [(1, CHUNK - 6, 2 * CHUNK + 11, 1, 2, 0)]


def _one_frame():
    return np.array([[-1, 1, -1]], dtype=np.int64), [(0, 0, 1, -1, -1, -1), (2, 0, 1, -1, -1, -1)]


def _before_equals_after():
    lab = _base(40)
    lab[10:20, 0] = -1
    lab[30:33, 0] = -1
    lab[33:, 0] = 5
    return lab, [(0, 10, 20, 0, 0, -1), (0, 30, 33, 0, 5, 0)]


HAND_BUILT = [_an_ion_never_assigned, _nobody_assigned, _a_run_from_frame_0, _a_run_to_the_last_frame,
              _a_run_covering_one_chunk_exactly, _runs_ending_and_starting_on_the_chunk_cut, _a_run_across_three_chunks,
              _one_frame, _before_equals_after]


@pytest.mark.parametrize("case", HAND_BUILT, ids=[c.__name__.strip("_") for c in HAND_BUILT])
def test_hand_built_cases(oracle, case):
    lab, records = case()
    exp = np.array(records, dtype=np.int64).reshape(-1, 6)
    assert np.array_equal(R.runs(lab)[0], exp)                  # first the brute force gives the records written down
    centers, pos = R.designed_geometry(lab.shape[0], lab.shape[1], seed=len(lab))
    rec = check_against_brute_force(oracle, lab, centers, pos)
    assert np.array_equal(rec, exp)
    # and with values carried in: the runs that touch an end of the frames take them
    before_in, after_in = R.halos(lab.shape[1], seed=1)
    check_against_brute_force(oracle, lab, centers, pos, before_in, after_in, frame0=7)


def test_no_frames():
    with Device(np.zeros((0, 3), dtype=np.int64)) as ctx:
        first, last = ctx.label_ends()
        assert (first == R.NONE).all() and (last == R.NONE).all() and first.shape == (3,)
        assert ctx.replace_unassigned(0).shape == (0, 3) and ctx.replace_unassigned(1).shape == (0, 3)
        rec, npos = ctx.unknown_runs()
        assert rec.shape == (0, 6) and npos == 0
        assert ctx.replace_closer(rec, np.zeros((2, 3)), np.zeros((0, 3))).shape == (0, 3)


def test_bad_arguments_are_refused():
    with Device(_base(10)) as ctx:
        with pytest.raises(ValueError):
            ctx.replace_unassigned(2)
        with pytest.raises(ValueError):
            ctx.replace_unassigned(0, before_in=np.zeros(2, dtype=np.int64))


# ---- 4. the closer-site strategy --------------------------------------------------------------------------------------

def _frac(*f):
    return np.asarray(f, dtype=np.float64) @ R.CELL


def test_nearer_only_through_a_periodic_image(oracle):
    """Site 0 at fractional (0.05, 0.5, 0.1), site 1 at (0.55, 0.5, 0.6) of the triclinic cell.  A position at
    (0.9, 0.5, 0.1) is nearer to site 0 only over the cell's a face, one at (0.05, 0.5, 0.95) only over its (tilted) c
    face: the plain Euclidean distance prefers the other site both times."""
    centers = np.array([_frac(0.05, 0.5, 0.1), _frac(0.55, 0.5, 0.6), _frac(0.3, 0.2, 0.3)])
    lab = np.array([[0, 1, 2], [-1, -1, -1], [-1, 0, -1], [1, 0, -1]], dtype=np.int64)
    pos = np.zeros((4, 3, 3))
    pos[1, 0], pos[2, 0], pos[1, 1] = _frac(0.9, 0.5, 0.1), _frac(0.5, 0.5, 0.55), _frac(0.05, 0.5, 0.95)
    for p in (pos[1, 0], pos[1, 1]):
        plain = np.linalg.norm(centers[:2] - p, axis=1)
        wrapped = oracle.distances(R.CELL, p, centers[:2])
        assert plain[0] > plain[1] + 0.5 and wrapped[0] < wrapped[1] - 0.5
    exp = np.array([[0, 1, 2], [0, 0, -1], [1, 0, -1], [1, 0, -1]])
    assert np.array_equal(R.closer(oracle, R.CELL, lab, centers, pos)[0], exp)
    with Device(lab) as ctx:
        rec, npos = ctx.unknown_runs()
        assert np.array_equal(rec, [(0, 1, 3, 0, 1, 0), (1, 1, 2, 1, 0, 2), (2, 1, 4, 2, -1, -1)]) and npos == 3
        assert np.array_equal(ctx.replace_closer(rec, centers, R.positions_of(rec, pos)), exp)   # ion 2: one side unknown
    # through the operator: ion j is atom j + 2 of the real trajectory
    from sitator_amd import ReplaceUnassignedPositions as RUP, SiteTrajectory
    st = SiteTrajectory(R.plain_network(3, centers), lab)
    with pytest.raises(ValueError):
        RUP(RUP.replace_with_closer()).run(st)                  # no real trajectory
    st.set_real_traj(R.real_trajectory(pos))
    assert np.array_equal(RUP(RUP.replace_with_closer()).run(st).traj, exp)


def test_a_label_beyond_the_sites_raises_index_error():
    from sitator_amd import ReplaceUnassignedPositions as RUP, SiteTrajectory
    lab = np.array([[0], [-1], [K + 2]], dtype=np.int64)
    centers, pos = R.designed_geometry(3, 1, seed=0)
    with Device(lab) as ctx:
        rec, npos = ctx.unknown_runs()
        assert np.array_equal(rec, [(0, 1, 2, 0, K + 2, 0)]) and npos == 1
        with pytest.raises(IndexError, match="index %d is out of bounds" % (K + 2)):
            ctx.replace_closer(rec, centers, pos[1])
    st = SiteTrajectory(R.plain_network(1, centers), lab)
    st.set_real_traj(R.real_trajectory(pos))
    with pytest.raises(IndexError):
        RUP(RUP.replace_with_closer()).run(st)


BAD_RECORDS = {
    "negative_ion": (-1, 2, 4, 0, 1, 0),
    "ion_past_the_last": (2, 2, 4, 0, 1, 0),
    "start_before_the_frames": (0, 99, 104, 0, 1, 0),
    "end_past_the_frames": (0, 108, 111, 0, 1, 0),
    "empty_run": (0, 104, 104, 0, 1, 0),
    "offset_past_the_end": (0, 102, 104, 0, 1, 3),
    "negative_offset": (0, 102, 104, 0, 1, -1),
    "site_below_unknown": (0, 102, 104, -2, 1, 0),
    "huge_numbers": (0, -(1 << 62), 1 << 62, 0, 1, 1 << 62),
}


@pytest.mark.parametrize("bad", sorted(BAD_RECORDS))
def test_malformed_records_are_refused(bad):
    """10 frames from frame 100, 2 ions, 4 positions: every record here breaks one bound and is refused with
    ValueError before anything is indexed with it; the good record alone passes."""
    lab = _base(10)
    lab[2:4, 0] = -1
    lab[4:, 0] = 1
    centers, _ = R.designed_geometry(1, 1, seed=0)
    positions = np.ones((4, 3))
    good = (0, 102, 104, 0, 1, 0)
    with Device(lab, frame0=100) as ctx:
        assert np.array_equal(ctx.unknown_runs()[0], [good])
        with pytest.raises(ValueError):
            ctx.replace_closer(np.array([good, BAD_RECORDS[bad]]), centers, positions)
        out = ctx.replace_closer(np.array([good]), centers, positions)
        assert np.array_equal(out[:, 1], lab[:, 1]) and set(out[2:4, 0]) <= {0, 1} and np.array_equal(out[4:, 0], lab[4:, 0])
        # a record that claims known frames fills nothing there
        out = ctx.replace_closer(np.array([(1, 100, 110, 0, 0, -1)]), centers, positions)
        assert np.array_equal(out, lab)


# ---- 5. frame shards ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3])
def test_gpu_frame_shards_equal_the_single_rank(oracle, n):
    """``ThreadComm.group(n)``, a thread and a context per rank on GPU 0, contiguous frame blocks; the middle shard of
    three holds no known label of ion 2, ion 4's run crosses both cuts."""
    lab, centers, pos, cuts = R.sharded_case()
    exp_closer, margin = R.closer(oracle, R.CELL, lab, centers, pos)
    assert margin >= R.MARGIN
    single, joined, failures = R.run_sharded(lab, centers, pos, cuts[n])
    assert not failures, failures
    assert np.array_equal(single[0], R.replace(lab, 0)) and np.array_equal(single[1], R.replace(lab, 1))
    assert np.array_equal(single[2], exp_closer)
    for k in range(3):
        assert np.array_equal(np.concatenate([part[k] for part in joined]), single[k]), k


def test_gpu_any_other_callable_on_frame_shards_is_refused():
    lab, centers, pos, cuts = R.sharded_case()
    _, _, failures = R.run_sharded(lab, centers, pos, cuts[2], custom=True)
    assert sorted(failures) == [(0, "NotImplementedError"), (1, "NotImplementedError")]


# ---- 6. after the landmark path: the labels are read where run() left them --------------------------------------------

def test_operator_reads_the_labels_where_run_left_them(oracle):
    from sitator_amd import (JumpAnalysis, LandmarkAnalysis, ReplaceUnassignedPositions as RUP, SiteNetwork,
                             SiteTrajectory, Structure, synth, _lib)
    host = synth.config_host("C1")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 500, seed=17, p_hop=1.0 / 40)
    sn = SiteNetwork(Structure(ref, host.cell), sm, mm)
    sn.centers = host.centers
    sn.vertices = host.vertices
    st = LandmarkAnalysis(verbose=False).run(sn, frames)
    assert st.n_unassigned > 0
    strategies = (None, RUP.replace_with_last_known, RUP.replace_with_next_known, RUP.replace_with_closer())

    uploads = []
    real = _lib.HipContext.set_assignments

    def counting(self, *a, **k):
        uploads.append(1)
        return real(self, *a, **k)

    version = st._ctx.labels_version
    _lib.HipContext.set_assignments = counting
    try:
        outs = [(RUP() if fn is None else RUP(fn)).run(st) for fn in strategies]
        assert len(uploads) == 0, "the labels run() left on the device must not be uploaded again"
    finally:
        _lib.HipContext.set_assignments = real
    assert st._ctx.labels_version == version
    lab = st._traj
    assert np.array_equal(outs[0].traj, R.replace(lab, 0)) and np.array_equal(outs[1].traj, outs[0].traj)
    assert np.array_equal(outs[2].traj, R.replace(lab, 1))
    mobile = frames[:, np.where(mm)[0]]
    exp, _ = R.closer(oracle, np.asarray(host.cell, dtype=np.float64), lab, np.asarray(st.site_network.centers), mobile)
    assert np.array_equal(outs[3].traj, exp)
    fresh = SiteTrajectory(st.site_network.copy(), lab.copy())
    assert np.array_equal(RUP().run(fresh).traj, outs[0].traj)
    for out in outs:
        assert out.real_trajectory is frames and np.shares_memory(out.confidences, st.confidences)
        JumpAnalysis().run(out)
        assert out.site_network.has_attribute("n_ij") and not st.site_network.has_attribute("n_ij")
