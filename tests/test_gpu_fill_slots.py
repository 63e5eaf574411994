"""k_fill3's two forms of a wave's window - the flat task space (SITATOR_F3_SLOT=0) and the slot form, a D0 lane per
(ion, slot of its candidate list) (SITATOR_F3_SLOT=1) - only differ in which lane tests which candidate: the sparse
rows, the error key, the zero-row count and the fused assignment must be identical bit for bit, on every shape of
window the slot form has a rule for.  sit_info [28] (`fill_slot_width`) says which form ran: 0 = flat, otherwise the
widest slots per ion a window of the launch could take."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOT_ENV = "SITATOR_F3_SLOT"


def _ctx(host, M, F, seed, mutate=None, midpoint=1.5):
    from sitator_amd import _lib, synth
    frames, sm, mm, ref = synth.make_trajectory(host, M, F, seed=seed)
    if mutate is not None:
        mutate(frames, sm, mm)
    ctx = _lib.HipContext(host.cell)
    ref_static = ref[sm]
    V = max(len(v) for v in host.vertices)
    verts = np.full((len(host.vertices), V), -1, dtype=np.int64)
    vcd = np.full(verts.shape, np.nan)
    for k, v in enumerate(host.vertices):
        verts[k, :len(v)] = v
        vcd[k, :len(v)] = ctx.distances(host.centers[k], ref_static[np.asarray(v)])
    ctx.set_basis(ref_static, verts, vcd, midpoint, 30, 1.0)
    ctx.set_frames(frames, np.where(sm)[0], np.where(mm)[0])
    return ctx, frames, sm, mm


def _pow2_slots(n):
    w = 8
    while w < n:
        w *= 2
    return w


def _with_env(env, fn):
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rows(ctx):
    nnz, idx, val = ctx.rows_sparse()
    live = np.arange(idx.shape[0])[:, None] < nnz[None, :]          # entries behind a row's length are whatever was there
    return nnz, np.where(live, idx, -1), np.where(live, val, 0.0)


def _fill_both(ctx, check_for_zeros=False, extra_env=None):
    """One fill in either form; returns the two results after requiring that they are equal and that each form ran."""
    out = []
    for slot in ("0", "1"):
        env = {SLOT_ENV: slot}
        env.update(extra_env or {})

        def run():
            rc, nz, err = ctx.fill(check_for_zeros=check_for_zeros)
            info = ctx.info()
            return rc, nz, (err.frame, err.index), info, _rows(ctx) if rc == 0 else None
        out.append(_with_env(env, run))
    (rc0, nz0, err0, info0, rows0), (rc1, nz1, err1, info1, rows1) = out
    assert info0["fill_kernel"] == 3 and info1["fill_kernel"] == 3
    assert info0["fill_slot_width"] == 0, "SITATOR_F3_SLOT=0 must run the flat task space"
    want = _pow2_slots(max(info1["tight_width"], info1["row_width"]) if info1["delta"] >= 0 else info1["row_width"])
    assert info1["fill_slot_width"] == want, "the slot form did not run where it is possible"
    assert (rc0, nz0, err0) == (rc1, nz1, err1)
    assert info0["fallback_frames"] == info1["fallback_frames"]
    if rc0 == 0:
        for a, b in zip(rows0, rows1):
            assert np.array_equal(a, b)
    return out


def _centres_from_rows(ctx):
    from sitator_amd.dotprod_classifier import DotProdClassifier, LandmarkVectors
    clf = DotProdClassifier(threshold=0.45)
    clf.fit_centers(LandmarkVectors(ctx))
    cen = np.asarray(clf.cluster_centers)
    ctx.set_centers(cen / np.linalg.norm(cen, axis=1)[:, None], True)


def _assign_both(ctx, extra_env=None):
    """The pass with the site assignment, as kernels of its own and fused into the fill, rows stored or not: labels,
    confidences and counts of the two forms are equal (and the stored rows)."""
    ref = None
    for fuse, store in (("0", True), ("1", True), ("1", False)):
        res = []
        for slot in ("0", "1"):
            env = {SLOT_ENV: slot, "SITATOR_FUSE": fuse}
            env.update(extra_env or {})

            def run():
                rc, nz, err = ctx.fill(check_for_zeros=False, assign=True, predict_threshold=0.8, store_rows=store)
                assert rc == 0
                info = ctx.info()
                return info, ctx.assignments(), _rows(ctx) if store else None
            res.append(_with_env(env, run))
        (i0, a0, r0), (i1, a1, r1) = res
        assert i0["fill_slot_width"] == 0 and i1["fill_slot_width"] > 0
        assert i0["assignment_fused"] == i1["assignment_fused"]
        for x, y in zip(a0, a1):
            assert np.array_equal(x, y), (fuse, store)
        if store:
            for x, y in zip(r0, r1):
                assert np.array_equal(x, y), (fuse, store)
        if ref is None:
            ref = a0
        for x, y in zip(ref, a1):
            assert np.array_equal(x, y), (fuse, store)


def test_c2_shape_takes_the_slot_form_by_default_and_both_forms_agree():
    """The benchmark's shape: 64 ions over four waves, windows of 16, no tight list longer than eight entries - the
    slot form is the default there (the test fails if the launch silently stays on the flat form)."""
    from sitator_amd import synth
    host = synth.config_host("C2")
    ctx, *_ = _ctx(host, 64, 200, seed=31)
    os.environ.pop(SLOT_ENV, None)
    rc, nz, err = ctx.fill()
    info = ctx.info()
    assert rc == 0 and info["fill_kernel"] == 3
    assert info["waves_per_workgroup"] == 4 and info["frames_per_workgroup"] == 1 and info["tight_width"] <= 8
    assert info["fill_slot_width"] > 0, "the slot form is the default where it is eligible"
    default_rows = _rows(ctx)
    out = _fill_both(ctx)
    for a, b in zip(default_rows, out[1][4]):
        assert np.array_equal(a, b)
    _centres_from_rows(ctx)
    _assign_both(ctx)
    rc, _, _ = _with_env({"SITATOR_FUSE": "1"}, lambda: ctx.fill(assign=True, predict_threshold=0.8, store_rows=False))
    info = ctx.info()
    assert rc == 0 and info["assignment_fused"] and info["fill_slot_width"] > 0


@pytest.mark.parametrize("midpoint,min_tight,slots,min_nnz", [(1.9, 9, 32, 5), (2.3, 17, 32, 9), (2.8, 33, 64, 17)])
def test_lists_longer_than_eight_slots_widen_the_slots_of_their_frame(midpoint, min_tight, slots, min_nnz):
    """A larger cut-off puts more landmarks in reach of a bin: the tight table's longest list outgrows eight slots (then
    16, then 32).  The rule is per frame: phase 1b records the longest list its ions met and the frame's windows run 16,
    32 or 64 slots per ion - sit_info reports the widest the launch could take (from the widest bin of the tight and of
    the fallback table)."""
    from sitator_amd import synth
    host = synth.config_host("C2")
    ctx, *_ = _ctx(host, 64, 60, seed=7, midpoint=midpoint)
    out = _fill_both(ctx)
    info = out[1][3]
    assert info["tight_width"] >= min_tight, "the case must have a tight list longer than the narrower slots"
    assert info["fill_slot_width"] == slots
    nnz = out[1][4][0]
    # rows wide enough for the wide-row assignment too; a row of more than 8 (16) entries also proves that a list of more
    # than 8 (16) candidates was walked by the slot form, i.e. that some frame ran 16 (32) or more slots per ion
    assert nnz.max() >= min_nnz
    _centres_from_rows(ctx)
    _assign_both(ctx)
    # few survivor slots and a small task table: windows drain in mid-window and spill
    _fill_both(ctx, extra_env={"SITATOR_FILL_RCAP": "8", "SITATOR_FILL_TCAP": "64"})


def test_ions_with_empty_lists_are_counted_or_raised_alike():
    from sitator_amd import synth, _lib
    host = synth.config_host("C2")

    def sit_on_host(frames, sm, mm):
        midx = np.where(mm)[0]
        frames[37, midx[5]] = host.static_pos[0] + 0.01             # no landmark in reach of these ions
        frames[37, midx[63]] = host.static_pos[9] + 0.01
        frames[80, midx[0]] = host.static_pos[100] - 0.01

    ctx, *_ = _ctx(host, 64, 120, seed=3, mutate=sit_on_host)
    out = _fill_both(ctx, check_for_zeros=False)
    assert out[1][0] == 0 and out[1][1] == 3
    out = _fill_both(ctx, check_for_zeros=True)
    assert out[1][0] == _lib.E_ZERO_LANDMARK and out[1][2] == (37, 5)


def test_frames_on_the_fallback_table_and_static_errors_agree():
    """A static atom beyond the sampled displacement bound sends its frame to the loose table (longer lists: the frame's
    windows pick their slot width from those); one beyond static_movement_threshold is the same error in both forms."""
    from sitator_amd import synth, _lib
    host = synth.config_host("C2")

    def shove(frames, sm, mm):
        sidx = np.where(sm)[0]
        frames[37, sidx[100]] += (0.55, -0.2, 0.1)                  # within static_movement_threshold, far beyond the jitter
        frames[39, sidx[7]] += (0.0, 0.0, 0.8)
        frames[3999, sidx[300]] += (0.0, 0.5, 0.0)
    # 4100 frames are sampled with a stride of two: odd frames are not in the sample
    ctx, frames, sm, mm = _ctx(host, 64, 4100, seed=9, mutate=shove)
    out = _fill_both(ctx)
    info = out[1][3]
    assert out[1][0] == 0 and info["fallback_frames"] == 3
    assert info["row_width"] > 8, "the fallback table must have lists longer than eight entries"
    _centres_from_rows(ctx)
    _assign_both(ctx)
    bad = frames.copy()
    sidx = np.where(sm)[0]
    bad[77, sidx[321]] += np.array([0.9, 0.7, 0.0])                 # 1.14 A: beyond static_movement_threshold
    ctx.set_frames(bad, sidx, np.where(mm)[0])
    out = _fill_both(ctx)
    assert out[1][0] == _lib.E_STATIC_THRESHOLD and out[1][2] == (77, 321)


@pytest.mark.parametrize("M,iw", [(57, "0"), (57, "12"), (57, "20"), (64, "4"), (30, "16")])
def test_short_last_window_and_several_windows_per_wave(M, iw):
    """57 ions in windows of 16 leave a last window of 9; windows of 12 give a wave a second, short window (and the
    assignment a kernel of its own); windows of 4 make every D0 pass half idle."""
    from sitator_amd import synth
    host = synth.config_host("C2")
    ctx, *_ = _ctx(host, M, 90, seed=23)
    extra = {"SITATOR_FILL_IW": iw, "SITATOR_FILL_FPB": "1"} if iw != "0" else {"SITATOR_FILL_FPB": "1"}
    _fill_both(ctx, extra_env=extra)
    _centres_from_rows(ctx)
    _assign_both(ctx, extra_env=extra)


@pytest.mark.parametrize("waves", ["8", "16"])
def test_wider_workgroups_take_the_slot_form_on_request(waves):
    from sitator_amd import synth
    host = synth.config_host("C2")
    ctx, *_ = _ctx(host, 64, 90, seed=29)
    out = _fill_both(ctx, extra_env={"SITATOR_FILL_WAVES": waves})
    assert out[1][3]["waves_per_workgroup"] == int(waves)
