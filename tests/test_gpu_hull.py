"""GPU: ``sit_grouped_hull_volumes`` (hull.hip, ``k_group_hull``), ``sit_grouped_work_fetch`` and ``SiteVolumes(hulls="device")``
against the numpy restatement of tests/hull_ref.py (which tests/test_hull_predicates.py pins, on the same inputs, to the host
build of the kernel's own headers, to qhull and to exact arithmetic) and against the reference's own volumes
(tests/golden/site_groups_known_answers.npz).

Tolerances.  A vertex set and a facet count have none.  A device volume against the exact volume of the restatement's facet
list (the device's own list where both are certified, which the equal vertex mask and facet count attest):
``hull_ref.volume_bound``, derived from the inputs.  Against qhull: ``hull_ref.QHULL_REL_TOL``, 64 times the difference
measured between qhull and the exact volume on these inputs (hull_ref.py has the figure)."""
import contextlib
import logging

import numpy as np
import pytest

from tests import group_ref as GR
from tests import hull_ref as HR

pytestmark = pytest.mark.gpu

GG = GR.GroupGoldens()


@contextlib.contextmanager
def grouped(sites):
    """(context, offsets, the working copy expected after step 0 of one recentring) of a designed grouping."""
    from sitator_amd import _lib
    labels, pos, off, work = HR.grouping(sites)
    ctx = _lib.HipContext(HR.CELL)
    try:
        ctx.set_assignments(labels)
        assert np.array_equal(ctx.group_by_site(len(sites), positions=pos, mobile_idx=np.arange(1)), off)
        yield ctx, off, work
    finally:
        ctx.close()


REFERENCE = {}


def reference(name):
    """Per site of a designed grouping: the restatement's result, qhull's, the exact volume and the bound - computed once."""
    if name not in REFERENCE:
        sites = HR.GROUPINGS[name]
        _, _, off, work = HR.grouping(sites)
        out = []
        for s in range(len(sites)):
            pts = work[off[s]:off[s + 1]]
            ref = HR.wrap(pts)
            qv, qvol = HR.qhull(pts)
            out.append({"ref": ref, "qhull_vertices": qv, "qhull_volume": qvol, "exact": HR.exact_volume(pts, ref["facets"]),
                        "bound": HR.volume_bound(pts, ref["facets"])})
        REFERENCE[name] = out
    return REFERENCE[name]


def test_plan_is_the_header_s():
    from sitator_amd import _lib
    cap, open_cap, block, lds = _lib.hull_plan()
    assert cap == HR.FACET_CAP >= 1024 and open_cap == cap + 2 and block == 256 and 0 < lds <= 64 * 1024


@pytest.mark.parametrize("name", sorted(HR.GROUPINGS))
def test_designed_shapes(name):
    sites = HR.GROUPINGS[name]
    K = len(sites)
    want = reference(name)
    with grouped(sites) as (ctx, off, work):
        ctx.grouped_recenter_step(0, 1, None)
        assert np.array_equal(ctx.grouped_work_fetch(0, int(off[-1])), work)
        assert np.array_equal(ctx.grouped_work_fetch(int(off[K - 1]), int(off[K] - off[K - 1])), work[off[K - 1]:])
        vols, status, nf, mask = ctx.grouped_hull_volumes(K, vertex_mask=True)
        again = ctx.grouped_hull_volumes(K, vertex_mask=True)
        print("%s: %d sites, %d points, most facets %d, hull kernel %.3f ms"
              % (name, K, off[-1], nf.max(), ctx.group_info()["hull_ms"]))
        assert np.array_equal(ctx.grouped_work_fetch(0, int(off[-1])), work)                # the kernel only reads
    assert [a.tobytes() for a in again] == [vols.tobytes(), status.tobytes(), nf.tobytes(), mask.tobytes()]
    assert status.dtype == nf.dtype == np.int32 and mask.dtype == np.uint8 and len(mask) == off[-1]
    assert np.array_equal(status, np.zeros(K, dtype=np.int32))
    worst = worst_q = 0.0
    for s in range(K):
        w = want[s]
        assert w["ref"]["status"] == HR.CLOSED
        pts = work[off[s]:off[s + 1]]
        got_v = np.nonzero(mask[off[s]:off[s + 1]])[0]
        if sites[s][0] == "doubled":
            assert {tuple(p) for p in pts[got_v]} == {tuple(p) for p in pts[w["qhull_vertices"]]}, s
            assert np.array_equal(got_v, w["ref"]["vertices"]), s                           # of equal points the first
        else:
            assert np.array_equal(got_v, w["qhull_vertices"]), s
        assert nf[s] == len(w["ref"]["facets"]), s
        err = abs(HR.Fraction(float(vols[s])) - w["exact"])
        assert err <= HR.Fraction(w["bound"]), (s, float(err), w["bound"])
        assert abs(vols[s] - w["qhull_volume"]) <= HR.QHULL_REL_TOL * w["qhull_volume"], s
        worst = max(worst, float(err / w["exact"]))
        worst_q = max(worst_q, abs(vols[s] - w["qhull_volume"]) / w["qhull_volume"])
    print("%s: largest relative error against the exact volume %.3g, against qhull %.3g" % (name, worst, worst_q))
    if name == "shell":
        assert nf[0] == 1196 and mask.sum() == 600


def flagged_trajectory():
    labels, pos, off, work = HR.grouping(HR.FLAGGED_SITES)
    K = len(HR.FLAGGED_SITES)
    return GR.CR.trajectory(HR.CELL, np.zeros((1, 3)), np.ones(1, dtype=bool), np.zeros((K, 3)), labels, pos)


def test_flagged_shapes_get_a_status_and_the_host_s_value():
    from sitator_amd import SiteVolumes
    K = len(HR.FLAGGED_SITES)
    with grouped(HR.FLAGGED_SITES) as (ctx, off, work):
        ctx.grouped_recenter_step(0, 1, None)
        vols, status, nf, _ = ctx.grouped_hull_volumes(K)
    assert np.array_equal(status, [s[3] for s in HR.FLAGGED_SITES]) and np.array_equal(status, [2, 1, 2, 3])
    assert np.all(np.isnan(vols)) and nf[1] == 0 and nf[3] == HR.FACET_CAP
    host = SiteVolumes().compute_accessable_volumes(flagged_trajectory(), n_recenterings=2)
    op = SiteVolumes(hulls="device")
    st = flagged_trajectory()
    dev = op.compute_accessable_volumes(st, n_recenterings=2)
    assert np.array_equal(dev, host) and np.array_equal(st.site_network.accessable_site_volumes, host)
    assert host[0] == 1.0 and np.isinf(host[1]) and np.isinf(host[2]) and np.isfinite(host[3])
    assert op.last_hull_status == {0: 0, 1: 2, 2: 4, 3: 2, 4: 0}


@pytest.mark.parametrize("nr", [1, 8])
@pytest.mark.parametrize("name", GG.names)
def test_device_hulls_against_the_reference(name, nr, caplog):
    from sitator_amd import SiteVolumes
    st = GG.trajectory(name)
    K = st.site_network.n_sites
    op = SiteVolumes(hulls="device")
    with caplog.at_level(logging.INFO, logger="sitator_amd.site_descriptors"):
        vols = op.compute_accessable_volumes(st, n_recenterings=nr)
    want = GG.get(name, "out_access_vol_r%d" % nr)
    rel = np.abs(vols - want) / want
    print("%s r%d: largest relative difference to the reference %.3g; %r" % (name, nr, rel.max(), op.last_hull_times))
    assert np.all(rel <= HR.QHULL_REL_TOL)
    assert np.array_equal(st.site_network.accessable_site_volumes, vols)
    assert op.last_hull_status == {0: K * nr, 1: 0, 2: 0, 3: 0, 4: 0}                          # nothing went to the host
    assert any("device hulls by status" in r.getMessage() for r in caplog.records)
    # the restatement on the reference's own recentred clouds: the same bytes
    off, rec = GG.get(name, "out_offsets"), GG.get(name, "out_recentered_r%d" % nr)
    mine = np.array([min(HR.wrap(rec[i, off[s]:off[s + 1]])["volume"] for i in range(nr)) for s in range(K)])
    assert np.array_equal(vols, mine)


def test_default_is_the_host_and_bit_equal_to_the_reference():
    import scipy
    from sitator_amd import SiteVolumes
    assert SiteVolumes().hulls == "host" and SiteVolumes().last_hull_status is None
    with pytest.raises(ValueError):
        SiteVolumes(hulls="gpu")
    if scipy.__version__ != GG.scipy_version:
        pytest.skip("hull volumes are compared exactly only with the scipy the goldens were made with (%s; installed: %s)"
                    % (GG.scipy_version, scipy.__version__))
    for name in GG.names:
        for nr in (1, 8):
            st = GG.trajectory(name)
            op = SiteVolumes(hulls="host")
            op.compute_accessable_volumes(st, n_recenterings=nr)
            assert np.array_equal(st.site_network.accessable_site_volumes, GG.get(name, "out_access_vol_r%d" % nr)), (name, nr)
            assert op.last_hull_status is None


@pytest.mark.parametrize("name", GG.names)
def test_empty_sites_shards_and_compute_volumes_are_unchanged(name):
    from sitator_amd import SiteVolumes

    class TwoRanks(object):
        size, rank = 2, 0

    st = GG.trajectory(name, labels_key="in_labels_empty")
    with pytest.raises(IndexError):
        SiteVolumes(hulls="device").compute_accessable_volumes(st)
    assert not st.site_network.has_attribute("accessable_site_volumes")
    st = GG.trajectory(name)
    st._comm = TwoRanks()
    with pytest.raises(NotImplementedError):
        SiteVolumes(hulls="device").compute_accessable_volumes(st)
    if GG.has(name, "in_vertices"):
        a, b = GG.network(name), GG.network(name)
        SiteVolumes().compute_volumes(a)
        SiteVolumes(hulls="device").compute_volumes(b)
        assert a.site_volumes.tobytes() == b.site_volumes.tobytes()
        assert a.site_surface_areas.tobytes() == b.site_surface_areas.tobytes()


def test_refused_before_step_0_and_for_a_stale_grouping():
    sites = HR.GROUPINGS["edges"]
    K = len(sites)
    labels = HR.grouping(sites)[0]
    with grouped(sites) as (ctx, off, work):
        with pytest.raises(ValueError, match="no working copy"):
            ctx.grouped_hull_volumes(K)
        with pytest.raises(ValueError, match="no working copy"):
            ctx.grouped_work_fetch(0, 1)
        ctx.grouped_recenter_step(0, 8, None)
        ctx.grouped_hull_volumes(K)
        with pytest.raises(ValueError, match="outside the grouping"):
            ctx.grouped_work_fetch(1, int(off[-1]))
        with pytest.raises(ValueError, match="number of sites"):
            ctx.grouped_hull_volumes(K + 1)
        ctx.set_assignments(labels)                                   # the same labels, written again
        with pytest.raises(ValueError, match="^stale"):
            ctx.grouped_hull_volumes(K)
        with pytest.raises(ValueError, match="^stale"):
            ctx.grouped_work_fetch(0, 1)
        # a new grouping has no working copy until its own step 0
        ctx.group_by_site(K, positions=HR.grouping(sites)[1], mobile_idx=np.arange(1))
        with pytest.raises(ValueError, match="no working copy"):
            ctx.grouped_hull_volumes(K)


def test_resident_frames_and_host_positions_give_the_same_bytes():
    from sitator_amd import synth
    from tests.test_gpu_group import context
    host = synth.config_host("C1")
    cell = np.asarray(host.cell, dtype=np.float64)
    S, F, M, K = len(host.static_pos), 130, 66, 9
    labels, pos, confs = GR.designed(cell, F, M, K, seed=12, n_unknown=300, consumers=False)
    mobile = GR.layout(M, S, "interleaved", seed=3)
    midx = np.where(mobile)[0]
    real = GR.embed(mobile, pos, seed=5, cell=cell)
    with context(frames=real, mobile_idx=midx) as ctx:
        ctx.set_assignments(labels, confs)
        results = []
        for kw in ({}, {"positions": real, "mobile_idx": midx}):
            ctx.group_by_site(K, **kw)
            for i in range(2):
                ctx.grouped_recenter_step(i, 2, None)
                results.append([a.tobytes() for a in ctx.grouped_hull_volumes(K, vertex_mask=True)])
        assert results[0] == results[2] and results[1] == results[3]


def test_for_analysis_equals_the_host_array_route():
    from sitator_amd import SiteVolumes
    from tests.test_gpu_group import analysis
    la, sn, frames = analysis()
    st = la.run(sn, frames)
    st.set_real_traj(frames)
    counts = st.group_real_positions(_resident=True).counts
    op = SiteVolumes(hulls="device")
    if counts.min() == 0:                                               # the analysis' own sites: they are what they are
        with pytest.raises(IndexError):
            op.compute_accessable_volumes(st)
        with pytest.raises(IndexError):
            op.compute_accessable_volumes_for_analysis(la)
    else:
        want = op.compute_accessable_volumes(st).copy()
        status = dict(op.last_hull_status)
        st.site_network.remove_attribute("accessable_site_volumes")
        assert op.compute_accessable_volumes_for_analysis(la).tobytes() == want.tobytes()
        assert op.last_hull_status == status
