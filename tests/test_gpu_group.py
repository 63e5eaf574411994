"""GPU: ``sit_group_by_site`` and the ``sit_grouped_*`` calls (group.hip), ``SiteTrajectory.group_real_positions``,
``NAvgsPerSite`` and ``SiteVolumes`` on top of them - against the numpy restatement of tests/group_ref.py computed in the same
process (which tests/test_group_ref.py pins to the TRUE reference) and against the reference's own outputs
(tests/golden/site_groups_known_answers.npz).

Grouping and recentring have no tolerance: positions, confidences and entry numbers are copies, a recentring step is one IEEE
add per coordinate and the wrap of clamp_point.h (pinned bit for bit by tests/test_clamp_point.py); the designed inputs keep
every floored crystal coordinate at least ``MARGIN`` from an integer.  A bucket average shifts and wraps the same way and then
sums in an order of its own: its bound is derived here from the inputs, per component
``4 * len(bucket) * 2^-52 * max|coordinate of the shifted, wrapped points|`` (``group_ref.bucket_bound``: the length times the
unit roundoff times the largest term bounds a sum of that many terms in any order, times 4 for the two-stage tree and the
division).  Buckets of one or two points are summed in the reference's own order and compared exactly."""
import contextlib

import numpy as np
import pytest

from tests import group_ref as GR

pytestmark = pytest.mark.gpu

GG = GR.GroupGoldens()
CELL = GR.TRICLINIC


def plan(n_entries=1, K=1):
    from sitator_amd import _lib
    return _lib.group_plan(n_entries, K)


CHUNK = None


def chunk():
    global CHUNK
    if CHUNK is None:
        CHUNK = plan()[0]
    return CHUNK


def shape_for(n):
    """(F, M) with F * M == n and M as wide as it comes below 300 (more ions than a wave where n allows)."""
    for M in range(299, 0, -1):
        if n % M == 0:
            return n // M, M


@contextlib.contextmanager
def context(cell=CELL, frames=None, mobile_idx=None):
    """A context, closed on exit.  ``frames``: made resident the way ``LandmarkAnalysis.run`` does it (tests/test_gpu_clamped.py:
    the basis of the smallest synthetic configuration first), with ``mobile_idx`` as the mobile columns."""
    from sitator_amd import _lib, synth
    if frames is None:
        ctx = _lib.HipContext(cell)
    else:
        host = synth.config_host("C1")
        ref_static = np.asarray(host.static_pos, dtype=np.float64)
        verts = np.full((len(host.vertices), max(len(v) for v in host.vertices)), -1, dtype=np.int64)
        for k, v in enumerate(host.vertices):
            verts[k, :len(v)] = v
        ctx = _lib.HipContext(host.cell)
        try:
            ctx.set_basis(ref_static, verts, ctx.site_vertex_distances(np.asarray(host.centers), ref_static, verts), 1.5, 30, 1.0)
            assert frames.shape[1] - len(mobile_idx) == len(ref_static)
            ctx.set_frames(frames, np.setdiff1d(np.arange(frames.shape[1]), mobile_idx), mobile_idx)
        except Exception:
            ctx.close()
            raise
    try:
        yield ctx
    finally:
        ctx.close()


def fetch_all(ctx, offsets):
    return ctx.grouped_fetch(0, int(offsets[-1]), True, True, True)


def assert_grouping(ctx, offsets, want, what=""):
    w_off, w_ent, w_pts, w_cf = want
    assert offsets.dtype == np.int64 and np.array_equal(offsets, w_off), what
    pts, cf, ent = fetch_all(ctx, offsets)
    assert np.array_equal(ent, w_ent), what
    assert np.array_equal(pts, w_pts), what
    assert np.array_equal(cf, w_cf), what


# ---- 1. the grouping ----------------------------------------------------------------------------------------------------------

def grouping_shapes():
    c = chunk()
    return [(1, 1, 1), (3, 7, 3), (5, 65, 30)] + [shape_for(n) + (5,) for n in (c - 1, c, c + 1)] + [(200, 70, 9), (3, 3, 5)]


@pytest.mark.parametrize("layout", ["first", "last", "interleaved"])
@pytest.mark.parametrize("case", range(8))
def test_grouping_against_restatement(case, layout):
    F, M, K = grouping_shapes()[case]
    labels, pos, confs = GR.designed(CELL, F, M, K, seed=F + M, n_unknown=F * M // 9, consumers=False)
    mobile = GR.layout(M, 3, layout, seed=M)
    midx = np.where(mobile)[0]
    real = GR.embed(mobile, pos, seed=F)
    want = GR.grouped(labels, K, real, midx, confs)
    print("F=%d M=%d K=%d: %d entries, %d chunks of %d" % (F, M, K, F * M, plan(F * M, K)[1], chunk()))
    with context() as ctx:
        ctx.set_assignments(labels, confs)
        version = ctx.labels_version
        for cap in (0, real.shape[1] * 24):                          # everything at once; one frame at a time
            assert_grouping(ctx, ctx.group_by_site(K, positions=real, mobile_idx=midx, workspace_bytes=cap), want, cap)
        assert np.array_equal(ctx.site_counts(K), np.diff(want[0]))
        # a part of the grouping, and nothing moved
        if want[0][-1] > 2:
            pts, cf, ent = ctx.grouped_fetch(1, int(want[0][-1]) - 2, True, True, True)
            assert np.array_equal(pts, want[2][1:-1]) and np.array_equal(cf, want[3][1:-1]) and np.array_equal(ent, want[1][1:-1])
        assert ctx.labels_version == version
        assert np.array_equal(ctx.assignments()[0].reshape(labels.shape), labels)


def test_one_site_over_several_chunks():
    F, M = 3 * chunk() // 64 + 5, 64
    labels, pos, confs = GR.designed(CELL, F, M, 1, seed=4, n_unknown=F * M // 5, consumers=False)
    assert plan(F * M, 1)[1] >= 3
    with context() as ctx:
        ctx.set_assignments(labels, confs)
        assert_grouping(ctx, ctx.group_by_site(1, positions=pos, mobile_idx=np.arange(M)), GR.grouped(labels, 1, pos, np.arange(M), confs))


def test_more_sites_than_entries_and_nothing_assigned():
    F, M, K = 3, 7, 100
    labels, pos, confs = GR.designed(CELL, F, M, K, seed=8, n_unknown=4, consumers=False)
    with context() as ctx:
        ctx.set_assignments(labels, confs)
        want = GR.grouped(labels, K, pos, np.arange(M), confs)
        assert np.count_nonzero(np.diff(want[0]) == 0) > K - F * M
        assert_grouping(ctx, ctx.group_by_site(K, positions=pos, mobile_idx=np.arange(M)), want)
        ctx.set_assignments(np.full((F, M), -1, dtype=np.int64), confs)
        off = ctx.group_by_site(K, positions=pos, mobile_idx=np.arange(M))
        assert np.array_equal(off, np.zeros(K + 1, dtype=np.int64))
        assert all(len(a) == 0 for a in fetch_all(ctx, off))
        assert np.array_equal(ctx.group_by_site(0, positions=pos, mobile_idx=np.arange(M)), [0])


def test_equal_labels_inside_a_tile_keep_their_order():
    """One site named by 2, 3 and 64 ions of one frame (multiple occupancy is legal input): their rank is the entry order."""
    F, M, K = 6, 70, 5
    labels, pos, confs = GR.designed(CELL, F, M, K, seed=21, consumers=False)
    labels[0, :64] = 2                                                # a whole tile of equal labels
    labels[1, :] = 4
    labels[1, [0, 31, 69]] = 1
    labels[2, :] = -1
    labels[2, [3, 40]] = 0
    labels[3, 6:] = 3                                                 # 64 ions across two tiles
    labels[4, :] = 2
    with context() as ctx:
        ctx.set_assignments(labels, confs)
        off = ctx.group_by_site(K, positions=pos, mobile_idx=np.arange(M))
        want = GR.grouped(labels, K, pos, np.arange(M), confs)
        assert_grouping(ctx, off, want)
        ent = fetch_all(ctx, off)[2]
        for s in range(K):
            assert np.all(np.diff(ent[off[s]:off[s + 1]]) > 0)


def test_sites_beyond_the_lds_form():
    limit = plan()[3]
    K = limit + 1
    assert plan(10, limit)[2] and not plan(10, K)[2]
    F, M = 150, 65
    assert plan(F * M, K)[1] >= 3
    rng = np.random.default_rng(6)
    labels, pos, confs = GR.designed(CELL, F, M, K, seed=6, n_unknown=500, consumers=False)
    few = rng.choice(K, size=7, replace=False)                         # equal labels inside tiles and across chunks
    sel = rng.uniform(size=labels.shape) < 0.5
    labels[sel & (labels >= 0)] = few[rng.integers(0, 7, size=np.count_nonzero(sel & (labels >= 0)))]
    labels[0, 0], labels[-1, -1] = K - 1, 0
    with context() as ctx:
        ctx.set_assignments(labels, confs)
        for cap in (0, M * 24):
            assert_grouping(ctx, ctx.group_by_site(K, positions=pos, mobile_idx=np.arange(M), workspace_bytes=cap),
                            GR.grouped(labels, K, pos, np.arange(M), confs))
        assert not ctx.group_info()["lds"]


@pytest.mark.parametrize("layout", ["first", "last", "interleaved"])
def test_resident_frames_and_host_positions_give_the_same_bytes(layout):
    from sitator_amd import _lib, synth
    from tests.test_gpu_clamped import resident_frames
    host = synth.config_host("C1")
    cell = np.asarray(host.cell, dtype=np.float64)
    S, F, M, K = len(host.static_pos), 130, 66, 9
    labels, pos, confs = GR.designed(cell, F, M, K, seed=12, n_unknown=300, consumers=False)
    mobile = GR.layout(M, S, layout, seed=3)
    midx = np.where(mobile)[0]
    real = GR.embed(mobile, pos, seed=5, cell=cell)
    want = GR.grouped(labels, K, real, midx, confs)
    with context(frames=real, mobile_idx=midx) as ctx:
        ctx.set_assignments(labels, confs)
        assert_grouping(ctx, ctx.group_by_site(K), want, "resident")
        a = [x.tobytes() for x in fetch_all(ctx, want[0])]
        assert_grouping(ctx, ctx.group_by_site(K, positions=real, mobile_idx=midx, workspace_bytes=real.shape[1] * 24 * 7), want, "host")
        assert a == [x.tobytes() for x in fetch_all(ctx, want[0])]
        assert np.array_equal(resident_frames(ctx), real)
        # shapes other than the resident ones
        with pytest.raises(ValueError):
            ctx.group_by_site(K, positions=real[:-1], mobile_idx=midx)
        with pytest.raises(ValueError):
            ctx.group_by_site(K, positions=real, mobile_idx=midx[:-1])
        off = np.zeros(K + 1, dtype=np.int64)
        assert ctx.lib.sit_group_by_site(ctx._h, None, F, real.shape[1] + 1, None, M, K, 0, _lib._i(off)) == _lib.E_INVALID


def test_bad_labels_caps_and_stale_groupings():
    F, M, K = 9, 5, 4
    labels, pos, confs = GR.designed(CELL, F, M, K, seed=3, n_unknown=5, consumers=False)
    midx = np.arange(M)
    with context() as ctx:
        with pytest.raises(ValueError):
            ctx.grouped_fetch(0, 0)                                   # no assignments, no grouping
        ctx.set_assignments(labels, confs)
        with pytest.raises(ValueError, match="no grouping"):
            ctx.grouped_fetch(0, 0)
        with pytest.raises(ValueError, match="no resident frames"):
            ctx.group_by_site(K)
        with pytest.raises(ValueError, match="below one frame"):
            ctx.group_by_site(K, positions=pos, mobile_idx=midx, workspace_bytes=M * 24 - 1)
        with pytest.raises(ValueError, match="mobile index"):
            ctx.group_by_site(K, positions=pos, mobile_idx=midx + 1)
        with pytest.raises(IndexError, match="index %d is out of bounds for axis 0 with size %d" % (K - 1, K - 1)):
            ctx.group_by_site(K - 1, positions=pos, mobile_idx=midx)
        with pytest.raises(ValueError, match="no grouping"):
            ctx.grouped_fetch(0, 0)                                   # a failed call leaves none behind
        bad = labels.copy()
        bad[4, 2] = -2
        ctx.set_assignments(bad, confs)
        with pytest.raises(ValueError, match="below -1"):
            ctx.group_by_site(K, positions=pos, mobile_idx=midx)
        ctx.set_assignments(labels, confs)
        off = ctx.group_by_site(K, positions=pos, mobile_idx=midx)
        with pytest.raises(ValueError, match="outside the grouping"):
            ctx.grouped_fetch(1, int(off[-1]))
        ctx.set_assignments(labels, confs)                            # the same labels, written again
        for call in (lambda: ctx.grouped_fetch(0, 1), lambda: ctx.grouped_bucket_averages(K, 2, True),
                     lambda: ctx.grouped_recenter_step(0, 8, None)):
            with pytest.raises(ValueError, match="^stale"):
                call()
        assert_grouping(ctx, ctx.group_by_site(K, positions=pos, mobile_idx=midx), GR.grouped(labels, K, pos, midx, confs))


# ---- 2. cumulative recentring ---------------------------------------------------------------------------------------------------

def recentring_case(lengths, seed):
    """One ion; the sites have the given numbers of points, in shuffled frame order."""
    K, F = len(lengths), int(sum(lengths))
    while True:
        rng = np.random.default_rng(seed)
        labels = rng.permutation(np.repeat(np.arange(K), lengths)).reshape(F, 1).astype(np.int64)
        pos = rng.uniform(-3.0, 4.0, size=(F, 1, 3)) @ CELL
        off, _, pts, _ = GR.grouped(labels, K, pos, np.arange(1))
        if GR.margin(CELL, off, pts, None, n_values=(), n_recenterings=(8,)) >= GR.MARGIN:
            return labels, pos, off, pts
        seed += 1000


def test_recentring_steps_are_bit_equal_and_so_are_the_volumes():
    from sitator_amd import SiteVolumes
    lengths = [1, 7, 8, 9, 40]                                        # the float index i * (len / 8) at len below, at and above 8
    labels, pos, off, pts = recentring_case(lengths, seed=2)
    with context() as ctx:
        ctx.set_assignments(labels)
        assert np.array_equal(ctx.group_by_site(len(lengths), positions=pos, mobile_idx=np.arange(1)), off)
        out = np.empty((int(off[-1]), 3))
        for i, want in enumerate(GR.recenter_steps(CELL, off, pts, 8)):
            assert ctx.grouped_recenter_step(i, 8, out) is out
            assert np.array_equal(out, want), i
        with pytest.raises(ValueError, match="in order"):
            ctx.grouped_recenter_step(3, 8, out)
        ctx.grouped_recenter_step(0, 1, out)                          # a new series starts from the grouped points
        assert np.array_equal(out, next(GR.recenter_steps(CELL, off, pts, 1)))
        assert np.array_equal(fetch_all(ctx, off)[0], pts)            # the grouping itself stays
    st = GR.CR.trajectory(CELL, np.zeros((1, 3)), np.ones(1, dtype=bool), np.zeros((len(lengths), 3)), labels, pos)
    vols = SiteVolumes().compute_accessable_volumes(st, n_recenterings=8)
    want = GR.accessible_volumes(CELL, off, pts, 8)
    assert np.array_equal(vols, want) and np.isinf(want[0]) and np.all(np.isfinite(want[1:]))
    assert np.array_equal(st.site_network.accessable_site_volumes, want)


def test_recentring_an_empty_site_fails_as_the_reference():
    assert str(GG.z["empty_site_error"]) == "IndexError"
    labels, pos, off, pts = recentring_case([5, 6, 4], seed=9)
    labels[labels == 1] = -1
    with context() as ctx:
        ctx.set_assignments(labels)
        ctx.group_by_site(3, positions=pos, mobile_idx=np.arange(1))
        with pytest.raises(IndexError, match="index 0 is out of bounds for axis 0 with size 0"):
            ctx.grouped_recenter_step(0, 8, None)


# ---- 3. bucket averages ------------------------------------------------------------------------------------------------------------

def bucket_case(n, seed, big):
    """Site lengths whose buckets pts[i::n] have 1, 2, 64, 65 and a few thousand points, plus a site that is not averaged."""
    lengths = [n + n // 2, 64 * n + n // 2, big * n + 1, n, 3 * n]
    K, F = len(lengths), int(sum(lengths))
    while True:
        rng = np.random.default_rng(seed)
        labels = rng.permutation(np.repeat(np.arange(K), lengths)).reshape(F, 1).astype(np.int64)
        pos = rng.uniform(-3.0, 4.0, size=(F, 1, 3)) @ CELL
        confs = (rng.permutation(F) / float(F) * 0.5 + 0.25).reshape(F, 1)              # distinct: no argmax tie
        off, _, pts, cf = GR.grouped(labels, K, pos, np.arange(1), confs)
        if GR.margin(CELL, off, pts, cf, n_values=(n,), n_recenterings=()) >= GR.MARGIN:
            return labels, pos, confs, off, pts, cf
        seed += 1000


@pytest.mark.parametrize("n", [2, 3, 4])                          # 3: an odd number of buckets
def test_bucket_averages_anchor_exact_and_mean_within_the_derived_bound(n):
    labels, pos, confs, off, pts, cf = bucket_case(n, seed=n, big=3000)
    K = len(off) - 1
    sizes = sorted({len(range(off[s] + i, off[s + 1], n)) for s in range(K) for i in range(n) if off[s + 1] - off[s] > n})
    assert {1, 2, 64, 65}.issubset(sizes) and sizes[-1] >= 3000
    assert len(np.unique(cf)) == len(cf)
    with context() as ctx:
        ctx.set_assignments(labels, confs)
        ctx.group_by_site(K, positions=pos, mobile_idx=np.arange(1))
        results = {}
        for weighted in (True, False):
            want, want_anchor = GR.bucket_averages(CELL, off, pts, cf, n, weighted)
            got, anchor = ctx.grouped_bucket_averages(K, n, weighted)
            results[weighted] = got
            assert np.array_equal(anchor, want_anchor)                                  # np.argmax of the weights / the first
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.all(np.isnan(got[3])) and not np.any(np.isnan(got[:3]))
            bound = GR.bucket_bound(CELL, off, pts, want_anchor, n)
            m = ~np.isnan(want)
            err = np.abs(got - want)
            print("n=%d weighted=%d: largest error %.3g, %.3g of its bound" % (n, weighted, err[m].max(), (err[m] / bound[m]).max()))
            assert np.all(err[m] <= bound[m])
            # one or two points: the reference's own order of operations, so the shifted points, the mean and its wrap are exact
            for s in range(K):
                for i in range(n):
                    if want_anchor[s, i] >= 0 and len(range(off[s] + i, off[s + 1], n)) <= 2:
                        assert np.array_equal(got[s, i], want[s, i]), (s, i)
        # a site's result does not depend on the other sites: take them away, one kind at a time
        for keep in ([2], [0, 2], [1, 2, 4]):
            ctx.set_assignments(np.where(np.isin(labels, keep), labels, -1), confs)
            ctx.group_by_site(K, positions=pos, mobile_idx=np.arange(1))
            for weighted in (True, False):
                got, _ = ctx.grouped_bucket_averages(K, n, weighted)
                for s in keep:
                    assert got[s].tobytes() == results[weighted][s].tobytes(), (keep, s)


# ---- 4. the operators end to end ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GG.names)
def test_site_grouping_is_real_positions_for_site(name):
    st = GG.trajectory(name)
    g = st.group_real_positions()
    K = st.site_network.n_sites
    assert g.n_sites == len(g) == K and np.array_equal(g.offsets, GG.get(name, "out_offsets"))
    assert np.array_equal(g.counts, st._device().site_counts(K))
    M = st.site_network.n_mobile
    for s in range(K):
        pts, confs = g.positions(s, return_confidences=True)
        want_pts, want_confs = st.real_positions_for_site(s, return_confidences=True)
        assert pts.flags["OWNDATA"] and np.array_equal(pts, want_pts) and np.array_equal(confs, want_confs)
        assert np.array_equal(g.positions(s), want_pts)
        e = g.entries(s)
        assert np.array_equal(st._traj.reshape(-1)[e], np.full(len(e), s)) and np.all(np.diff(e) > 0)
        assert np.array_equal(st.real_trajectory[e // M, np.where(st.site_network.mobile_mask)[0][e % M]], pts)
    assert np.array_equal(np.concatenate([g.positions(s) for s in range(K)]), GG.get(name, "out_points"))
    # the grouping belongs to the labels it was made from
    st.assign_to_last_known_site(frame_threshold=10 ** 6)
    with pytest.raises(ValueError, match="^stale"):
        g.positions(0)
    bare = GG.trajectory(name, with_confs=False)
    with pytest.raises(ValueError, match="no confidences"):
        bare.group_real_positions().positions(0, return_confidences=True)
    bare.remove_real_traj()
    with pytest.raises(ValueError, match="^This SiteTrajectory has no real trajectory$"):
        bare.group_real_positions()
    single = GG.trajectory(name)
    single.set_real_traj(single.real_trajectory.astype(np.float32))
    with pytest.raises(ValueError, match="expected 'double'"):
        single.group_real_positions()


@pytest.mark.parametrize("name", GG.names)
def test_navgs_per_site_against_the_reference(name):
    from sitator_amd import NAvgsPerSite
    cell, K = GG.get(name, "in_cell"), len(GG.get(name, "in_centers"))
    midx = np.where(GG.get(name, "in_mobile_mask"))[0]
    off, _, pts, cf = GR.grouped(GG.get(name, "in_labels"), K, GG.get(name, "in_real"), midx, GG.get(name, "in_confs"))
    for weighted in (0, 1):
        for n in (2, 4):
            sn = NAvgsPerSite(n, weighted=bool(weighted)).run(GG.trajectory(name, with_confs=bool(weighted)))
            want = GG.get(name, "out_navg_w%d_n%d_centers" % (weighted, n))
            _, anchors = GR.bucket_averages(cell, off, pts, cf, n, bool(weighted))
            bound = GR.bucket_bound(cell, off, pts, anchors, n).reshape(-1, 3)
            err = np.abs(np.asarray(sn.centers) - want)
            print("%s weighted=%d n=%d: largest error %.3g, %.3g of its bound" % (name, weighted, n, err.max(), (err / bound).max()))
            assert sn.centers.shape == want.shape and np.all(err <= bound)
            assert np.array_equal(sn.site_types, GG.get(name, "out_navg_w%d_n%d_types" % (weighted, n)))
            assert sn.n_mobile == len(midx)
    # a site with 3 points and n = 4
    st = GG.trajectory(name, labels_key="in_labels_few")
    with pytest.raises(ValueError) as info:
        NAvgsPerSite(4).run(st)
    assert "ValueError: %s" % info.value == str(GG.get(name, "out_navg_few_n4_error"))
    sn = NAvgsPerSite(4, error_on_insufficient=False).run(st)
    want = GG.get(name, "out_navg_few_n4_centers")
    assert np.array_equal(sn.site_types, GG.get(name, "out_navg_few_n4_types"))
    assert np.array_equal(np.asarray(sn.centers)[-3:], want[-3:])                       # the site's own points, in order
    off, _, pts, cf = GR.grouped(GG.get(name, "in_labels_few"), K, GG.get(name, "in_real"), midx, GG.get(name, "in_confs"))
    _, anchors = GR.bucket_averages(cell, off, pts, cf, 4, True)
    bound = GR.bucket_bound(cell, off, pts, anchors, 4)[:K - 1].reshape(-1, 3)
    assert np.all(np.abs(np.asarray(sn.centers)[:-3] - want[:-3]) <= bound)
    # the reference's other errors
    with pytest.raises(AssertionError):
        NAvgsPerSite(3)
    with pytest.raises(ValueError, match="no confidences"):
        NAvgsPerSite(2).run(GG.trajectory(name, with_confs=False))
    st.remove_real_traj()
    with pytest.raises(ValueError, match="^SiteTrajectory must have associated real trajectory.$"):
        NAvgsPerSite(2).run(st)


@pytest.mark.parametrize("name", GG.names)
def test_site_volumes_errors_and_attributes(name):
    from sitator_amd import InsufficientCoordinatingAtomsError, SiteVolumes
    st = GG.trajectory(name, labels_key="in_labels_empty")
    with pytest.raises(IndexError):                                     # the class the goldens record
        SiteVolumes().compute_accessable_volumes(st)
    assert not st.site_network.has_attribute("accessable_site_volumes")
    st = GG.trajectory(name)
    SiteVolumes().run(st)
    assert st.site_network.accessable_site_volumes.shape == (st.site_network.n_sites,)
    if not GG.has(name, "in_vertices"):
        with pytest.raises(ValueError, match="must have verticies"):
            SiteVolumes().compute_volumes(st.site_network)
        st.site_network.vertices = [[] for _ in range(st.site_network.n_sites)]
        with pytest.raises(InsufficientCoordinatingAtomsError, match="Site 0 had only 0 vertices"):
            SiteVolumes().compute_volumes(st.site_network)
        SiteVolumes(error_on_insufficient_coord=False).compute_volumes(st.site_network)
        assert np.all(st.site_network.site_volumes == 0) and np.all(np.isnan(st.site_network.site_surface_areas))


def test_site_volumes_against_the_reference():
    import scipy
    from sitator_amd import SiteVolumes
    if scipy.__version__ != GG.scipy_version:
        pytest.skip("hull volumes are compared exactly only with the scipy the goldens were made with (%s; installed: %s)"
                    % (GG.scipy_version, scipy.__version__))
    for name in GG.names:
        for nr in (1, 8):
            st = GG.trajectory(name)
            SiteVolumes().compute_accessable_volumes(st, n_recenterings=nr)
            assert np.array_equal(st.site_network.accessable_site_volumes, GG.get(name, "out_access_vol_r%d" % nr)), (name, nr)
        if GG.has(name, "in_vertices"):
            sn = GG.network(name)
            SiteVolumes().compute_volumes(sn)
            assert np.array_equal(sn.site_volumes, GG.get(name, "out_site_volumes"))
            assert np.array_equal(sn.site_surface_areas, GG.get(name, "out_site_surface_areas"))


def analysis():
    from sitator_amd import LandmarkAnalysis, SiteNetwork, Structure, synth
    host = synth.config_host("C1")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 300, seed=17, p_hop=1.0 / 40)
    sn = SiteNetwork(Structure(ref, host.cell), sm, mm)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False)
    return la, sn, frames


def test_operators_for_analysis_equal_the_host_path():
    from sitator_amd import NAvgsPerSite, SiteTrajectory, SiteVolumes
    from tests.test_gpu_clamped import resident_frames
    la, sn, frames = analysis()
    with pytest.raises(ValueError):
        NAvgsPerSite(2).run_for_analysis(la)                            # has not run
    st = la.run(sn, frames)
    st.set_real_traj(frames)
    labels, version = st._traj.copy(), la._ctx.labels_version
    for weighted in (True, False):
        op = NAvgsPerSite(2, error_on_insufficient=False, weighted=weighted)
        want = op.run(st)
        for got in (op.run_for_analysis(la), op.run_for_analysis(la, st)):
            assert np.array_equal(got.centers, want.centers) and np.array_equal(got.site_types, want.site_types)
    counts = st.group_real_positions(_resident=True).counts
    print("site counts: min %d max %d over %d sites" % (counts.min(), counts.max(), len(counts)))
    if counts.min() == 0:                                               # the analysis' own sites: they are what they are
        with pytest.raises(IndexError):
            SiteVolumes().compute_accessable_volumes(st)
        with pytest.raises(IndexError):
            SiteVolumes().compute_accessable_volumes_for_analysis(la)
    else:
        want = SiteVolumes().compute_accessable_volumes(st).copy()
        st.site_network.remove_attribute("accessable_site_volumes")
        assert np.array_equal(SiteVolumes().compute_accessable_volumes_for_analysis(la), want)
    # nothing moved
    assert la._ctx.labels_version == version and np.array_equal(st._traj, labels)
    assert np.array_equal(resident_frames(la._ctx), frames)
    assert np.array_equal(la._ctx.assignments()[0].reshape(labels.shape), labels)
    foreign = SiteTrajectory(st.site_network, labels)
    foreign.set_real_traj(frames)
    with pytest.raises(ValueError, match="does not share"):
        NAvgsPerSite(2, error_on_insufficient=False).run_for_analysis(la, foreign)


def test_frame_shards_are_refused():
    from sitator_amd import NAvgsPerSite, SiteVolumes

    class TwoRanks(object):
        size, rank = 2, 0

    name = GG.names[0]
    st = GG.trajectory(name)
    st._comm = TwoRanks()
    with pytest.raises(NotImplementedError):
        st.group_real_positions()
    with pytest.raises(NotImplementedError):
        NAvgsPerSite(2).run(st)
    with pytest.raises(NotImplementedError):
        SiteVolumes().compute_accessable_volumes(st)
    la, sn, frames = analysis()
    la.run(sn, frames)
    la._comm = TwoRanks()
    with pytest.raises(NotImplementedError):
        NAvgsPerSite(2).run_for_analysis(la)
    with pytest.raises(NotImplementedError):
        SiteVolumes().compute_accessable_volumes_for_analysis(la)
