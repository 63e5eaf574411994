"""GPU: ``sit_clamp_trajectory`` (clamp.hip) and ``GenerateClampedTrajectory`` on top of it, against the numpy restatement
of tests/clamp_ref.py (which tests/test_clamp_ref.py pins to the TRUE reference) and against the reference's own outputs
(tests/golden/clamped_known_answers.npz).

There is no tolerance anywhere: every compared value is a copy or a fixed sequence of IEEE multiply, add and floor
operations that the library evaluates without contraction, so equality is bitwise.  The square root enters only the
choice among the 27 images; the designed inputs keep the two nearest images at least ``MARGIN`` apart and every floored
crystal coordinate at least ``MARGIN`` from an integer (``clamp_ref.designed`` steps its seed until that holds, and the
tests assert it).

Shapes: one element; a few; more atoms than a wave (65); a frame that is not a multiple of the 256-element tile and an odd
number of doubles (257 x 70 ... 1000 x 130: several hundred workgroups, frames that straddle tiles)."""
import ctypes

import numpy as np
import pytest

from tests import clamp_ref as CR

pytestmark = pytest.mark.gpu

CG = CR.ClampGoldens()
SHAPES = [(1, 1, 1), (3, 7, 3), (5, 65, 30), (257, 70, 33), (1000, 130, 60)]       # (F, A, M)


class Context(object):
    """A context (closed on exit).  ``frames``: made resident the way ``LandmarkAnalysis.run`` does it - the basis of the
    smallest synthetic configuration first, then the frames, whose leading atoms stand for the basis' static ones."""

    def __init__(self, cell=None, frames=None):
        self.cell, self.frames = cell, frames

    def __enter__(self):
        from sitator_amd import _lib, synth
        if self.frames is None:
            self.ctx = _lib.HipContext(self.cell)
            return self.ctx
        host = synth.config_host("C1")
        ref_static = np.asarray(host.static_pos, dtype=np.float64)
        verts = np.full((len(host.vertices), max(len(v) for v in host.vertices)), -1, dtype=np.int64)
        for k, v in enumerate(host.vertices):
            verts[k, :len(v)] = v
        self.ctx = _lib.HipContext(host.cell)
        try:
            vcd = self.ctx.site_vertex_distances(np.asarray(host.centers), ref_static, verts)
            self.ctx.set_basis(ref_static, verts, vcd, 1.5, 30, 1.0)
            S, A = len(ref_static), self.frames.shape[1]
            assert A > S
            self.ctx.set_frames(self.frames, np.arange(S), np.arange(S, A))
        except Exception:
            self.ctx.close()
            raise
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()


def resident_frames(ctx):
    """The frames in the context's device memory, copied back by the HIP runtime itself."""
    hip = ctx.lib
    out = np.empty((ctx.F, ctx.A, 3))
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ctx.synchronize()
    assert hip.hipMemcpy(out.ctypes.data, ctx.frames_device_ptr(), out.nbytes, 2) == 0
    return out


def roles(mobile, clamp_mask):
    role = np.where(clamp_mask, -2, -1).astype(np.int32)
    sel = clamp_mask & mobile
    role[sel] = (np.cumsum(mobile) - 1)[sel]
    return role


def masks(mobile, seed):
    A = len(mobile)
    return {"all": np.ones(A, dtype=bool), "none": np.zeros(A, dtype=bool), "static": ~mobile, "mobile": mobile.copy(),
            "random": np.random.default_rng(seed).uniform(size=A) < 0.5}


# ---- 1. the entry point against the restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["first", "last", "interleaved"])
@pytest.mark.parametrize("F,A,M", SHAPES)
def test_entry_point_against_restatement(F, A, M, layout):
    cell, K = CR.TRICLINIC, 7
    centers, labels, pos = CR.designed(cell, F, M, K, seed=F + A, n_unknown=0)
    _, unknown, _ = CR.designed(cell, F, M, K, seed=F + A, n_unknown=max(1, F * M // 9))
    assert np.array_equal(np.where(unknown == -1, labels, unknown), labels)           # the same draw, some entries unknown
    m_img, m_floor = CR.margins(cell, centers, labels, pos)
    print("F=%d A=%d M=%d: image margin %.3g, floor margin %.3g" % (F, A, M, m_img, m_floor))
    assert m_img >= CR.MARGIN and m_floor >= CR.MARGIN
    crystal = CR.to_cell(cell, centers)
    assert F * M < 20 or (crystal.min() < 0 and crystal.max() > 1 and CR.to_cell(cell, pos).min() < -1)
    mobile, spos = CR.structure(M, A - M, layout, seed=A)
    real = CR.embed(mobile, spos, pos, seed=F)
    every = np.ones(A, dtype=bool)
    with Context(cell) as ctx:
        for p, lab in ((False, labels), (True, unknown)):
            ctx.set_assignments(lab)
            for w in (False, True):
                full = CR.clamp(cell, spos, mobile, centers, lab, real, every, w, p)
                for mname, mask in masks(mobile, seed=A + 1).items():
                    want = np.where(mask[None, :, None], full, real)
                    got = ctx.clamp_trajectory(roles(mobile, mask), spos, centers, w, p, positions=real)
                    assert got.dtype == np.float64 and got.shape == (F, A, 3)
                    assert np.array_equal(got, want), (w, p, mname)
        # nothing but labels and centres is needed: no positions at all
        ctx.set_assignments(labels)
        got = ctx.clamp_trajectory(roles(mobile, every), spos, centers, True, False)
        assert np.array_equal(got, CR.clamp(cell, spos, mobile, centers, labels, None, every, True, False))


def test_one_site_and_negative_images():
    cell = CR.ORTHO
    F, M = 40, 3
    centers, labels, pos = CR.designed(cell, F, M, 1, seed=77)
    pos = pos - 5.0 * cell.sum(axis=0)                             # every position in a negative image
    assert min(CR.margins(cell, centers, labels, pos)) >= CR.MARGIN and np.all(labels == 0)
    assert CR.to_cell(cell, pos).max() < 0
    mobile = np.ones(M, dtype=bool)
    with Context(cell) as ctx:
        ctx.set_assignments(labels)
        for w, p in CR.COMBOS:
            got = ctx.clamp_trajectory(np.arange(M), np.zeros((M, 3)), centers, w, p, positions=pos)
            assert np.array_equal(got, CR.clamp(cell, np.zeros((M, 3)), mobile, centers, labels, pos, None, w, p))


# ---- 2. host positions against resident frames -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resident_case():
    from sitator_amd import synth
    cell = np.asarray(synth.config_host("C1").cell, dtype=np.float64)
    F, S, M, K = 301, 27, 6, 5
    centers, labels, pos = CR.designed(cell, F, M, K, seed=12, n_unknown=40)
    mobile = np.arange(S + M) >= S
    spos = np.random.default_rng(2).uniform(size=(S + M, 3)) @ cell
    real = CR.embed(mobile, spos, pos, seed=6)
    return cell, centers, labels, mobile, spos, real


def test_resident_frames_against_host_positions(resident_case):
    cell, centers, labels, mobile, spos, real = resident_case
    with Context(frames=real) as ctx:
        ctx.set_assignments(labels)
        version = ctx.labels_version
        for mname, mask in masks(mobile, seed=3).items():
            role = roles(mobile, mask)
            for w in (False, True):
                host = ctx.clamp_trajectory(role, spos, centers, w, True, positions=real)
                assert np.array_equal(host, CR.clamp(cell, spos, mobile, centers, labels, real, mask, w, True)), (mname, w)
                assert np.array_equal(ctx.clamp_trajectory(role, spos, centers, w, True), host), (mname, w)
        # the call reads only
        assert ctx.labels_version == version
        assert np.array_equal(resident_frames(ctx), real)
        assert np.array_equal(ctx.assignments()[0].reshape(labels.shape), labels)
        with pytest.raises(ValueError):                            # A is not the resident frames'
            ctx.clamp_trajectory(roles(mobile, mobile)[:-1], spos[:-1], centers, False, True)


# ---- 3. chunking ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [6, 7])                             # a frame of an odd (33 atoms) and of an even number of doubles
def test_chunking_does_not_change_a_frame(M):
    from sitator_amd import synth
    cell = np.asarray(synth.config_host("C1").cell, dtype=np.float64)
    F, S = 301, 27
    centers, labels, pos = CR.designed(cell, F, M, 5, seed=40 + M, n_unknown=40)
    mobile = np.arange(S + M) >= S
    spos = np.random.default_rng(2).uniform(size=(S + M, 3)) @ cell
    real = CR.embed(mobile, spos, pos, seed=6)
    A = len(mobile)
    role = roles(mobile, np.ones(A, dtype=bool))
    frame_bytes = A * 24
    with Context(frames=real) as ctx:
        ctx.set_assignments(labels)
        want = ctx.clamp_trajectory(role, spos, centers, False, True, positions=real)           # the default cap
        assert np.array_equal(want, CR.clamp(cell, spos, mobile, centers, labels, real, None, False, True))
        for frames_per_chunk in (F, (F + 1) // 2, 7, 2, 1):       # 1, 2, an uneven number of chunks; one frame a chunk
            for per_frame, positions in ((2 * frame_bytes, real), (frame_bytes, None)):
                got = ctx.clamp_trajectory(role, spos, centers, False, True, positions=positions,
                                           workspace_bytes=frames_per_chunk * per_frame + 5)
                assert np.array_equal(got, want), (frames_per_chunk, positions is None)
        for per_frame, positions in ((2 * frame_bytes, real), (frame_bytes, None)):
            with pytest.raises(ValueError, match="below one frame"):
                ctx.clamp_trajectory(role, spos, centers, False, True, positions=positions, workspace_bytes=per_frame - 1)
        assert np.array_equal(ctx.clamp_trajectory(role, spos, centers, False, True), want)


# ---- 4. the reference's outputs through the public class --------------------------------------------------------------------------

@pytest.mark.parametrize("name", CG.names)
def test_reference_outputs_through_the_class(name):
    from sitator_amd import GenerateClampedTrajectory as GCT
    i = CG.inputs(name)
    cell = i["cell"]
    M = i["labels"].shape[1]
    all_mobile = np.ones(M, dtype=bool)
    for key, w, p, mask, with_real, expected in CG.outputs(name):
        st = CR.trajectory(cell, i["ref_positions"], all_mobile, i["centers"], i[key], i["positions"] if with_real else None)
        got = GCT(wrap=w, pass_through_unassigned=p).run(st, clamp_mask=mask)
        assert got.dtype == np.float64 and np.array_equal(got, expected), (key, w, p)
    for w in (False, True):
        st = CR.trajectory(cell, i["ref_positions"], all_mobile, i["centers"], i["labels_unassigned"], i["positions"])
        with pytest.raises(RuntimeError, match="unassigned at some point"):
            GCT(wrap=w).run(st)
    # the same labels on a structure with static atoms between the mobile ones
    mobile, spos = CR.structure(M, 4, "interleaved", seed=21)
    real = CR.embed(mobile, spos, i["positions"], seed=22)
    mask = np.random.default_rng(23).uniform(size=len(mobile)) < 0.6
    for w, p in CR.COMBOS:
        key = "labels_unassigned" if p else "labels"
        for m in (None, mask):
            st = CR.trajectory(cell, spos, mobile, i["centers"], i[key], real)
            got = GCT(wrap=w, pass_through_unassigned=p).run(st, clamp_mask=m)
            assert np.array_equal(got, CR.clamp(cell, spos, mobile, i["centers"], i[key], real, m, w, p)), (w, p)


def test_class_without_a_real_trajectory():
    from sitator_amd import GenerateClampedTrajectory as GCT
    i = CG.inputs("triclinic_big")
    M = i["labels"].shape[1]
    mobile, spos = CR.structure(M, 3, "last", seed=1)
    every = np.ones(len(mobile), dtype=bool)

    def st(key):
        return CR.trajectory(i["cell"], spos, mobile, i["centers"], i[key], None)

    want = CR.clamp(i["cell"], spos, mobile, i["centers"], i["labels"], None, every, True, False)
    assert np.array_equal(GCT(wrap=True).run(st("labels")), want)
    assert np.array_equal(GCT(wrap=True, pass_through_unassigned=True).run(st("labels")), want)      # nothing to pass through
    # a mask without a mobile atom is valid (the reference: numpy's ValueError for the minimum of nothing)
    assert str(CG.z["empty_mask_error"]) == "ValueError"
    real = CR.embed(mobile, spos, i["positions"], seed=2)
    for mask in (~mobile, np.zeros(len(mobile), dtype=bool)):
        got = GCT().run(CR.trajectory(i["cell"], spos, mobile, i["centers"], i["labels_unassigned"], real), clamp_mask=mask)
        assert np.array_equal(got, np.where(mask[None, :, None], spos[None], real))
    with pytest.raises(RuntimeError, match="leaves some atoms unclamped"):
        GCT(wrap=True).run(st("labels"), clamp_mask=mobile)
    with pytest.raises(RuntimeError, match="no real-space trajectory"):
        GCT(wrap=False).run(st("labels"))
    with pytest.raises(RuntimeError, match="no real-space trajectory"):
        GCT(wrap=True, pass_through_unassigned=True).run(st("labels_unassigned"))
    with pytest.raises(RuntimeError, match="unassigned at some point"):
        GCT(wrap=True).run(st("labels_unassigned"))
    t = CR.trajectory(i["cell"], spos, mobile, i["centers"], i["labels"],
                      np.zeros((len(i["labels"]), len(mobile), 3), dtype=np.float32))
    with pytest.raises(ValueError, match="expected 'double'"):
        GCT().run(t)


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable():
    from sitator_amd import errors
    cell, K = CR.TRICLINIC, 4
    F, M = 600, 3
    centers, labels, pos = CR.designed(cell, F, M, K, seed=31)
    mobile = np.ones(M, dtype=bool)
    role = np.arange(M, dtype=np.int32)
    fixed = np.zeros((M, 3))
    want = CR.clamp(cell, fixed, mobile, centers, labels, pos, None, False, False)
    frame_bytes = M * 24

    with Context(cell) as ctx:
        def good():
            ctx.set_assignments(labels)
            assert np.array_equal(ctx.clamp_trajectory(role, fixed, centers, False, False, positions=pos), want)

        good()
        # unassigned entries in several chunks and columns: the smallest frame * M + column is reported
        bad = labels.copy()
        bad[[599, 450, 450, 123], [0, 2, 1, 2]] = -1
        ctx.set_assignments(bad)
        for w in (False, True):
            for cap in (0, 100 * 2 * frame_bytes):
                with pytest.raises(errors.UnassignedClampError) as e:
                    ctx.clamp_trajectory(role, fixed, centers, w, False, positions=pos, workspace_bytes=cap)
                assert isinstance(e.value, RuntimeError) and e.value.first_unassigned == 123 * M + 2
        # ... only columns that are clamped count
        with pytest.raises(errors.UnassignedClampError) as e:
            ctx.clamp_trajectory(np.array([0, -1, -1], dtype=np.int32), fixed, centers, False, False, positions=pos)
        assert e.value.first_unassigned == 599 * M
        good()
        bad = labels.copy()
        bad[300, 1] = K + 2
        ctx.set_assignments(bad)
        with pytest.raises(IndexError, match="index %d is out of bounds" % (K + 2)):
            ctx.clamp_trajectory(role, fixed, centers, False, False, positions=pos)
        with pytest.raises(IndexError):
            ctx.clamp_trajectory(role, fixed, centers, True, True, positions=pos)
        good()
        bad = labels.copy()
        bad[5, 0] = -2
        ctx.set_assignments(bad)
        with pytest.raises(ValueError, match="below -1"):
            ctx.clamp_trajectory(role, fixed, centers, False, True, positions=pos)
        good()
        with pytest.raises(ValueError, match="number of frames"):
            ctx.clamp_trajectory(role, fixed, centers, False, False, positions=pos[:-1])
        for r in ([0, 1, M], [0, 1, -3], [0, 1, 1]):              # outside [-2, M), twice the same column
            with pytest.raises(ValueError):
                ctx.clamp_trajectory(np.array(r, dtype=np.int32), fixed, centers, False, False, positions=pos)
        with pytest.raises(ValueError, match="no resident frames"):
            ctx.clamp_trajectory(role, fixed, centers, False, False)
        good()


# ---- 6. straight from a LandmarkAnalysis -----------------------------------------------------------------------------------------

def test_run_for_analysis():
    from sitator_amd import (GenerateClampedTrajectory as GCT, JumpAnalysis, LandmarkAnalysis, SiteNetwork, SiteTrajectory,
                             Structure, synth)
    host = synth.config_host("C1")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 300, seed=17, p_hop=1.0 / 40)
    sn = SiteNetwork(Structure(ref, host.cell), sm, mm)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False)
    op = GCT(wrap=False, pass_through_unassigned=True)
    with pytest.raises(ValueError):
        op.run_for_analysis(la)                                                         # has not run
    st = la.run(sn, frames)
    ctx = la._ctx
    labels = st._traj.copy()
    JumpAnalysis().run(st)
    n_ij = np.array(st.site_network.n_ij)
    version = ctx.labels_version
    cell = np.asarray(host.cell, dtype=np.float64)
    centers = np.asarray(st.site_network.centers)
    mask = np.random.default_rng(5).uniform(size=frames.shape[1]) < 0.7
    for w, p in ((False, True), (True, True)):
        for m in (None, mask, mm):
            want = GCT(wrap=w, pass_through_unassigned=p).run(st, clamp_mask=m)
            assert np.array_equal(GCT(wrap=w, pass_through_unassigned=p).run_for_analysis(la, clamp_mask=m), want)
            assert np.array_equal(GCT(wrap=w, pass_through_unassigned=p).run_for_analysis(la, st, clamp_mask=m), want)
            margin = min(CR.margins(cell, centers, labels, frames[:, mm]))
            print("wrap %s: margin %.3g" % (w, margin))
            if w or margin >= CR.MARGIN:                     # the analysis' own centres: the margin is what it is
                assert np.array_equal(want, CR.clamp(cell, ref, mm, centers, labels, frames, m, w, p))
    # nothing moved
    assert ctx.labels_version == version
    assert np.array_equal(resident_frames(ctx), frames)
    assert np.array_equal(ctx.assignments()[0].reshape(labels.shape), labels) and np.array_equal(st._traj, labels)
    JumpAnalysis().run(st)
    assert np.array_equal(np.array(st.site_network.n_ij), n_ij)
    # a later state of the same trajectory: its new labels are the ones clamped
    st.assign_to_last_known_site(frame_threshold=10 ** 6)
    later = st._traj.copy()
    got = op.run_for_analysis(la, st)
    assert np.array_equal(got, op.run(st))
    assert np.array_equal(got[:, mm][later >= 0], GCT(wrap=False).run(
        CR.trajectory(cell, ref, mm, centers, np.where(later >= 0, later, 0), frames))[:, mm][later >= 0])
    assert np.array_equal(resident_frames(ctx), frames)
    # a trajectory with a context of its own
    foreign = SiteTrajectory(st.site_network, later)
    foreign.set_real_traj(frames)
    with pytest.raises(ValueError, match="does not share"):
        op.run_for_analysis(la, foreign)
    assert np.array_equal(op.run(foreign), got)


def test_run_for_analysis_refuses_recentred_frames_and_shards():
    from sitator_amd import GenerateClampedTrajectory as GCT, LandmarkAnalysis, RecenterTrajectory, SiteNetwork, Structure, synth
    host = synth.config_host("C1b")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 200, seed=31, p_hop=1.0 / 50)
    masses = np.random.default_rng(4).uniform(1.0, 40.0, size=frames.shape[1])
    ref_rec = ref[None].copy()
    RecenterTrajectory().run(Structure(ref, host.cell), sm, ref_rec, masses=masses)   # the basis recentred the same way
    sn = SiteNetwork(Structure(ref_rec[0], host.cell), sm, mm)
    sn.centers = np.asarray(host.centers) + (ref_rec[0, 0] - ref[0])
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False, recenter_masses=masses)
    la.run(sn, frames)
    with pytest.raises(ValueError, match="recent"):
        GCT(pass_through_unassigned=True).run_for_analysis(la)
    host = synth.config_host("C1")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 200, seed=3, p_hop=1.0 / 50)
    sn = SiteNetwork(Structure(ref, host.cell), sm, mm)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False, devices=[0, 0])
    la.run(sn, frames)
    with pytest.raises(NotImplementedError):
        GCT(pass_through_unassigned=True).run_for_analysis(la)
