"""GPU: ``sit_vanhove`` (vanhove.hip: the fractional coordinates, the distinct part over tiles of both selections, the self part on
the unwrapped series of msd.hip, the LDS histograms and their flush) and ``VanHoveCorrelation`` / ``RadialDistribution`` on top of
it, against the numpy restatement of tests/vanhove_ref.py (itself pinned to brute force and closed forms by
tests/test_vanhove_ref.py and to vanhove_plan.h by tests/test_vanhove_plan.py).

The counts are compared with ``np.array_equal`` on uint64: every decision is the same float64 operation sequence on both sides.
Inputs are random walks as in tests/test_gpu_msd.py, wrapped into cells whose heights are at least 3.  From the restatement
alone every case first asserts ``max_residual < 0.25`` (``wrapped_walk``) and, unless it is marked as degenerate (one frame, one
bin, one pair), that each part has a non-zero count in at least three bins and in the overflow entry, so that a result that is
all overflow cannot pass."""
import logging

import numpy as np
import pytest

from tests import golden_util as G
from tests import msd_ref as R
from tests import vanhove_ref as V
from tests.test_gpu_msd import Context, DRIFT, wrapped_walk
from tests.test_gpu_vibfreq import resident_frames

pytestmark = pytest.mark.gpu


def r_limit(cell, share=1.0):
    return 0.5 * V.hmin(cell) * V.MARGIN * share


def reference(x, cell, a, b, same, lags, stride, r_max, n_bins, unwrap=True):
    sc, res = V.self_part(x, cell, a, lags, stride, r_max, n_bins, unwrap=unwrap)
    return sc, V.distinct(x, cell, a, b, same, lags, stride, r_max, n_bins), res


def rich(table):
    total = table.sum(axis=0)
    return np.count_nonzero(total[:-1]) >= 3 and total[-1] > 0


def check_row_sums(sc, dc, F, lags, stride, n_a, n_b, same):
    origins = np.array([V.n_origins(F, int(t), stride) for t in lags], dtype=np.uint64)
    if sc is not None:
        assert np.array_equal(sc.sum(axis=1), origins * np.uint64(n_a))
    if dc is not None:
        assert np.array_equal(dc.sum(axis=1), origins * np.uint64(n_a * n_b - (n_a if same else 0)))


def device(ctx, x, a, b, same, lags, stride, r_max, n_bins, **kw):
    from sitator_amd import _lib_vanhove
    return _lib_vanhove.vanhove(ctx, a, b, lags, r_max, n_bins, positions=x, same=same, origin_stride=stride, **kw)


def lags_of(F, extra=()):
    return np.unique(np.clip([0, 1, F - 1] + list(extra), 0, F - 1))


# (cell, F, n_a, n_b or None for one selection, n_bins, stride, further lags, share of the largest r_max, degenerate)
CASES = {
    "one_frame": ("ortho", 1, 5, None, 16, 1, (), 1.0, True),
    "one_pair_one_bin": ("ortho", 2, 1, 1, 1, 1, (), 1.0, True),
    "one_atom_alone": ("hex", 3, 1, None, 16, 1, (), 1.0, True),
    "lanes_past_64": ("hex", 97, 5, 70, 16, 1, (5, 20, 50), 1.0, False),
    "one_selection_stride_3": ("triclinic", 400, 33, None, 300, 3, (7, 60, 200), 1.0, False),
    "one_selection_past_64": ("hex", 50, 70, None, 16, 1, (3, 20), 0.5, False),     # the left-out pair in the second tile of both lists
    "runs_of_origins": ("ortho", 400, 33, 200, 16, 1, (57,), 0.9, False),
    "one_atom_against_many": ("triclinic", 130, 1, 70, 16, 3, (9, 40), 0.6, False),
    "stride_beyond_the_frames": ("hex", 97, 5, 70, 16, 1000, (5, 20), 1.0, True),
    "two_lists_of_the_same_atoms": ("triclinic", 60, 33, -1, 16, 1, (4, 30), 0.8, False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_are_the_restatement(name):
    cell_name, F, n_a, n_b, n_bins, stride, extra, share, degenerate = CASES[name]
    cell = R.CELLS[cell_name]
    same = n_b is None
    total = n_a + (n_b if n_b and n_b > 0 else 0)
    x, _, _ = wrapped_walk(F, total, 100 + F + n_a, cell, drift=DRIFT)
    a = np.arange(n_a)
    b = a if (same or n_b < 0) else n_a + np.arange(n_b)
    lags, r_max = lags_of(F, extra), r_limit(cell, share)
    sc, dc, res = reference(x, cell, a, b, same, lags, stride, r_max, n_bins)
    assert degenerate or (rich(sc) and rich(dc))
    check_row_sums(sc, dc, F, lags, stride, n_a, len(b), same)
    with Context(cell) as ctx:
        got = device(ctx, x, a, b, same, lags, stride, r_max, n_bins)
        again = device(ctx, x, a, b, same, lags, stride, r_max, n_bins)
        plain = device(ctx, x, a, b, same, lags, stride, r_max, n_bins, unwrap=False, distinct_part=False)
        only_d = device(ctx, x, a, b, same, lags, stride, r_max, n_bins, self_part=False)
    assert got[0].dtype == got[1].dtype == np.uint64
    assert np.array_equal(got[0], sc) and np.array_equal(got[1], dc) and got[2] == res
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()          # two calls, the same bytes
    assert np.array_equal(plain[0], V.self_part(x, cell, a, lags, stride, r_max, n_bins, unwrap=False)[0])
    assert plain[1] is None and plain[2] == 0.0 and only_d[0] is None and np.array_equal(only_d[1], dc)
    if n_b is not None and n_b < 0:                               # every atom meets itself once per origin, at distance 0
        assert dc[0, 0] >= V.n_origins(F, 0, stride) * n_a and lags[0] == 0


def test_more_atoms_of_b_than_a_workgroup_takes():
    """33 atoms against 31 800: the plan gives a workgroup 31 744 atoms of b, so b is tiled over grid.z and the last tile is
    ragged; three frames keep the restatement short."""
    from sitator_amd import _lib_vanhove
    cell = R.TRICLINIC
    F, n_a, n_b = 3, 33, 31800
    plan = _lib_vanhove.vanhove_plan(F, n_a, n_b, 3, 16, self_part=False)
    assert plan["b_span"] == V.split(n_a, n_b)[1] == 31744 and plan["b_tiles"] == 2
    x = np.ascontiguousarray(np.random.default_rng(7).random((F, n_a + n_b, 3)) @ cell)
    a, b, lags, r_max = np.arange(n_a), n_a + np.arange(n_b), np.array([0, 1, 2]), r_limit(cell)
    dc = V.distinct(x, cell, a, b, False, lags, 1, r_max, 16)
    assert rich(dc)
    check_row_sums(None, dc, F, lags, 1, n_a, n_b, False)
    with Context(cell) as ctx:
        got = device(ctx, x, a, b, False, lags, 1, r_max, 16, self_part=False)
    assert np.array_equal(got[1], dc)


@pytest.fixture(scope="module")
def crowd():
    """F = 97, 140 atoms wrapped into the cell resident frames come with; the reference of two lists of them, computed once."""
    cell = Context.resident_cell()
    assert np.all(R.heights(cell) >= 3.0)
    x, _, _ = wrapped_walk(97, 140, 33, cell, drift=DRIFT)
    a, b = np.array([3, 17, 40, 41, 99]), np.concatenate([np.arange(50, 110), np.arange(120, 130)])
    lags, r_max, n_bins = lags_of(97, (5, 20, 50)), r_limit(cell, 0.15), 16    # the walk leaves a small r_max within 97 frames
    sc, dc, res = reference(x, cell, a, b, False, lags, 1, r_max, n_bins)
    assert rich(sc) and rich(dc)
    for arr in (x, sc, dc):
        arr.flags.writeable = False
    return dict(cell=cell, x=x, a=a, b=b, lags=lags, r_max=r_max, n_bins=n_bins, sc=sc, dc=dc, res=res)


def test_resident_frames_are_the_host_array(crowd):
    """The lists as columns of the resident frames (the other atoms holding NaN) and of the same array on the host: bit for bit, and
    the context stays as it was."""
    c = crowd
    mask = np.zeros(140, dtype=bool)
    mask[c["a"]] = mask[c["b"]] = True
    holed = np.where(mask[None, :, None], c["x"], np.nan)
    with Context(frames=holed) as ctx:
        version = ctx.labels_version
        host = device(ctx, holed, c["a"], c["b"], False, c["lags"], 1, c["r_max"], c["n_bins"])
        res = device(ctx, None, c["a"], c["b"], False, c["lags"], 1, c["r_max"], c["n_bins"])
        assert ctx.labels_version == version and np.array_equal(resident_frames(ctx), holed, equal_nan=True)
    for got in (host, res):
        assert np.array_equal(got[0], c["sc"]) and np.array_equal(got[1], c["dc"]) and got[2] == c["res"]


@pytest.mark.parametrize("stride", [1, 3])
def test_a_small_workspace_is_the_default(crowd, stride):
    """A cap of five frames' fractional coordinates (windows of five frames, a lag at a time; the series of one atom at a time)
    and one of a single frame: the same counts as with every frame held."""
    c = crowd
    frame = (len(c["a"]) + len(c["b"])) * 24
    sc, dc, res = (c["sc"], c["dc"], c["res"]) if stride == 1 else reference(c["x"], c["cell"], c["a"], c["b"], False, c["lags"], stride,
                                                                            c["r_max"], c["n_bins"])
    assert V.window(97, 5, 70, 512 + 5 * frame) == 5 and V.self_batch(97, 5, True, 512 + 5 * frame) == 1
    with Context(c["cell"]) as ctx:
        whole = device(ctx, c["x"], c["a"], c["b"], False, c["lags"], stride, c["r_max"], c["n_bins"])
        five = device(ctx, c["x"], c["a"], c["b"], False, c["lags"], stride, c["r_max"], c["n_bins"], workspace_bytes=512 + 5 * frame)
        one = device(ctx, c["x"], c["a"], c["b"], False, c["lags"], stride, c["r_max"], c["n_bins"], workspace_bytes=512 + frame,
                     self_part=False)
        with pytest.raises(ValueError):
            device(ctx, c["x"], c["a"], c["b"], False, c["lags"], stride, c["r_max"], c["n_bins"], workspace_bytes=511 + frame, self_part=False)
        with pytest.raises(ValueError):                           # the series of one atom do not fit
            device(ctx, c["x"], c["a"], c["b"], False, c["lags"], stride, c["r_max"], c["n_bins"], workspace_bytes=512 + frame)
    assert np.array_equal(whole[0], sc) and np.array_equal(whole[1], dc) and whole[2] == res
    assert whole[0].tobytes() == five[0].tobytes() and whole[1].tobytes() == five[1].tobytes() and five[2] == res
    assert whole[1].tobytes() == one[1].tobytes()


def test_per_wave_histograms_count_the_same(crowd, monkeypatch):
    c = crowd
    monkeypatch.setenv("SITATOR_VANHOVE_HIST_COPIES", "4")
    with Context(c["cell"]) as ctx:
        got = device(ctx, c["x"], c["a"], c["b"], False, c["lags"], 1, c["r_max"], c["n_bins"])
    assert np.array_equal(got[0], c["sc"]) and np.array_equal(got[1], c["dc"])


def test_designed_pairs():
    """An atom exactly on another (r2 = 0: bin 0); a pair at exactly half a cell vector (ds = 1/2: the tie rounds to even, the
    distance is 2 and lies beyond r_max); a NaN coordinate, which moves its own pairs to the overflow and no other."""
    cell = R.ORTHO                                               # 4 x 3.5 x 5
    r_max, n_bins = r_limit(cell), 16
    F = 20
    x, _, _ = wrapped_walk(F, 12, 5, cell)
    x = np.array(x)
    x[:, 7] = x[:, 2]                                            # atom 7 rides on atom 2
    x[:, 8] = [0.5, 1.0, 1.0]
    x[:, 9] = [2.5, 1.0, 1.0]                                    # s = 0.125 and 0.625 along the first cell vector: ds = 1/2 exactly
    a, b, lags = np.arange(0, 6), np.arange(6, 12), np.array([0, 3])
    sc, dc, res = reference(x, cell, a, b, False, lags, 1, r_max, n_bins, unwrap=False)
    assert rich(dc) and dc[0, 0] >= F
    pair = V.distinct(x, cell, [8], [9], False, [0], 1, r_max, n_bins)[0]
    assert pair[n_bins] == F and pair[:n_bins].sum() == 0
    dirty = x.copy()
    dirty[4, 2, 1] = np.nan                                      # atom 2 of list a, frame 4
    dirty[11, 9, 0] = np.inf                                     # atom 9 of list b, frame 11
    dsc, ddc, _ = reference(dirty, cell, a, b, False, lags, 1, r_max, n_bins, unwrap=False)
    assert np.all(ddc[:, :n_bins] <= dc[:, :n_bins]) and np.array_equal(ddc.sum(axis=1), dc.sum(axis=1)) and not np.array_equal(ddc, dc)
    assert np.array_equal(dsc.sum(axis=1), sc.sum(axis=1)) and dsc[0, n_bins] == 1 and dsc[1, n_bins] == sc[1, n_bins] + 2
    with Context(cell) as ctx:
        got = device(ctx, x, a, b, False, lags, 1, r_max, n_bins, unwrap=False)
        got_pair = device(ctx, x, [8], [9], False, [0], 1, r_max, n_bins, self_part=False)
        got_dirty = device(ctx, dirty, a, b, False, lags, 1, r_max, n_bins, unwrap=False)
        unwrapped = device(ctx, dirty, a, b, False, lags, 1, r_max, n_bins)
    assert np.array_equal(got[0], sc) and np.array_equal(got[1], dc)
    assert np.array_equal(got_pair[1][0], pair)
    assert np.array_equal(got_dirty[0], dsc) and np.array_equal(got_dirty[1], ddc)
    usc, _, ures = reference(dirty, cell, a, b, False, lags, 1, r_max, n_bins)
    assert np.array_equal(unwrapped[0], usc) and unwrapped[2] == ures and np.array_equal(unwrapped[1], ddc)


def test_limits_are_errors_not_faults(crowd):
    from sitator_amd import _lib_vanhove
    c = crowd
    ok = dict(a=c["a"], b=c["b"], same=False, lags=c["lags"], stride=1, r_max=c["r_max"], n_bins=c["n_bins"])

    def call(ctx, x, **kw):
        args = dict(ok, **kw)
        extra = {k: args.pop(k) for k in ("self_part", "distinct_part", "workspace_bytes") if k in args}
        return device(ctx, x, args["a"], args["b"], args["same"], args["lags"], args["stride"], args["r_max"], args["n_bins"], **extra)

    half = 0.5 * V.hmin(c["cell"])
    with Context(frames=np.array(c["x"])) as ctx:
        assert np.array_equal(call(ctx, None)[1], c["dc"])
        for bad in (dict(lags=[97]), dict(lags=[-1]), dict(lags=[0, 1 << 40]), dict(lags=[]), dict(stride=0), dict(stride=-3),
                    dict(n_bins=0), dict(n_bins=-1), dict(n_bins=V.MAX_BINS + 1), dict(a=[0, 140]), dict(b=[-1]), dict(a=[3, 1 << 40]),
                    dict(a=[]), dict(b=[]), dict(same=True), dict(r_max=0.0), dict(r_max=-1.0), dict(r_max=half), dict(r_max=np.nan),
                    dict(r_max=np.inf), dict(r_max=np.nextafter(r_limit(c["cell"]), 1e9)), dict(self_part=False, distinct_part=False),
                    dict(workspace_bytes=100), dict(workspace_bytes=-1)):
            with pytest.raises(ValueError):
                call(ctx, None, **bad)
        assert call(ctx, None, n_bins=V.MAX_BINS, lags=[0, 96], self_part=False)[1].shape == (2, V.MAX_BINS + 1)
        with pytest.raises(ValueError):                          # F other than the resident frames'
            ctx.F += 1
            try:
                call(ctx, None)
            finally:
                ctx.F -= 1
        with pytest.raises(ValueError):                          # no frame at all
            _lib_vanhove.vanhove(ctx, [0], [1], [0], 1.0, 4, positions=np.zeros((0, 2, 3)))
        assert np.array_equal(call(ctx, None)[0], c["sc"])       # and the context still works
    with Context(c["cell"]) as ctx:
        with pytest.raises(ValueError):                          # nothing resident
            call(ctx, None)


def test_a_degenerate_cell_is_refused():
    from sitator_amd import VanHoveCorrelation
    traj = R.random_walk(20, 2, seed=61)
    flat = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]])
    for cell in (flat, np.zeros((3, 3))):
        with pytest.raises(ValueError):                          # numpy's inverse refuses it, or sit_vanhove does
            VanHoveCorrelation([0, 1], 0.5, 4).compute(traj, cell, [0, 1])


def analysis(recenter=False):
    from sitator_amd import LandmarkAnalysis, SiteNetwork, Structure, synth
    host = synth.config_host("C1b")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 300, seed=31, p_hop=1.0 / 50)
    sn = SiteNetwork(Structure(ref, host.cell), sm, mm)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False)
    la.run(sn, frames)
    return la, np.ascontiguousarray(frames), np.asarray(host.cell, dtype=np.float64), sm, mm


def test_operators_on_the_frames_an_analysis_left_resident(caplog):
    from sitator_amd import RadialDistribution, RDFResult, VanHoveCorrelation, VanHoveResult
    la, frames, cell, sm, mm = analysis()
    F, n_bins = len(frames), 24
    r_max = r_limit(cell, 0.95)
    mobile, static = np.where(mm)[0], np.where(sm)[0]
    lags = [0, 1, 10, 100]
    sc, dc, res = reference(frames, cell, mobile, mobile, True, np.array(lags), 2, r_max, n_bins)
    assert res < 0.25 and rich(sc) and rich(dc)
    op = VanHoveCorrelation(lags, r_max, n_bins, origin_stride=2)
    version = la._ctx.labels_version
    with caplog.at_level(logging.WARNING, logger="sitator_amd.dynamics"):
        got = op.compute_for_analysis(la)
        host = op.compute(frames, cell, mm)
    assert not caplog.records and isinstance(got, VanHoveResult)
    for r in (got, host, op.compute_for_analysis(la, mask=mm), op.compute_for_analysis(la, mask=mobile)):
        assert np.array_equal(r.self_counts, sc) and np.array_equal(r.distinct_counts, dc) and r.max_residual == res
    origins = np.array([V.n_origins(F, t, 2) for t in lags])
    assert np.array_equal(got.n_origins, origins) and np.array_equal(got.lags, lags)
    dr = r_max / n_bins
    assert np.array_equal(got.edges[:-1], np.arange(n_bins) * dr) and got.edges[-1] == r_max
    assert np.array_equal(got.r, 0.5 * (got.edges[:-1] + got.edges[1:]))
    assert np.array_equal(got.self_density, sc[:, :n_bins] / (origins[:, None] * 4 * dr))
    shells = 4.0 * np.pi / 3.0 * (got.edges[1:] ** 3 - got.edges[:-1] ** 3)
    np.testing.assert_allclose(got.distinct, dc[:, :n_bins] * abs(np.linalg.det(cell)) / (origins[:, None] * 12 * shells[None, :]), rtol=1e-14)
    # two selections, and the radial distribution of the framework around the ions
    ms = VanHoveCorrelation([0, 5], r_max, n_bins, self_part=False).compute_for_analysis(la, mask_b=sm)
    assert ms.self_counts is None and ms.self_density is None
    assert np.array_equal(ms.distinct_counts, V.distinct(frames, cell, mobile, static, False, [0, 5], 1, r_max, n_bins))
    rdf = RadialDistribution(r_max, n_bins, frame_stride=3)
    g = rdf.compute_for_analysis(la)
    exp = V.distinct(frames, cell, mobile, static, False, [0], 3, r_max, n_bins)[0]
    assert isinstance(g, RDFResult) and rich(exp[None]) and np.array_equal(g.counts, exp) and g.n_origins == V.n_origins(F, 0, 3)
    assert np.array_equal(g.n, np.cumsum(exp[:n_bins]) / (g.n_origins * 4.0))
    np.testing.assert_allclose(g.g, exp[:n_bins] * abs(np.linalg.det(cell)) / (g.n_origins * 4 * len(static) * shells), rtol=1e-14)
    h = rdf.compute(frames, cell, mm, sm)
    assert np.array_equal(h.counts, exp) and np.array_equal(h.g, g.g)
    mm_rdf = rdf.compute_for_analysis(la, mask_b=None)
    assert np.array_equal(mm_rdf.counts, V.distinct(frames, cell, mobile, mobile, True, [0], 3, r_max, n_bins)[0])
    with pytest.raises(ValueError):
        rdf.compute_for_analysis(la, mask_b="mobile")
    with pytest.raises(IndexError):
        op.compute_for_analysis(la, mask=[frames.shape[1]])
    with pytest.raises(ValueError, match="Buffer dtype mismatch"):
        op.compute(frames.astype(np.float32), cell, mm)
    with pytest.raises(ValueError):
        VanHoveCorrelation(lags, 0.5 * V.hmin(cell) * 1.01, n_bins).compute_for_analysis(la)
    assert la._ctx.labels_version == version and np.array_equal(resident_frames(la._ctx), frames)
    # steps of 0.3 cell vectors: one warning, from the self part only
    jumpy = (np.arange(12)[:, None, None] * 0.3 * cell[0][None, None, :]) + np.zeros((12, 2, 3))
    with caplog.at_level(logging.WARNING, logger="sitator_amd.dynamics"):
        r = VanHoveCorrelation([1], r_max, 4).compute(jumpy, cell, [0, 1])
        VanHoveCorrelation([1], r_max, 4, self_part=False).compute(jumpy, cell, [0, 1])
    assert len(caplog.records) == 1 and 0.25 < r.max_residual <= 0.5


def test_operators_refuse_frame_shards():
    from sitator_amd import LandmarkAnalysis, RadialDistribution, SiteNetwork, Structure, VanHoveCorrelation
    c = G.Case("c1_hex_scgrid")
    sn = SiteNetwork(Structure(c.ref_positions, c.cell), c.static_mask, c.mobile_mask)
    sn.centers = c.centers
    sn.vertices = c.vertices
    la = LandmarkAnalysis(verbose=False, devices=[0, 0], **c.kwargs("dotprod"))
    la.run(sn, np.ascontiguousarray(c.frames))
    with pytest.raises(NotImplementedError):
        VanHoveCorrelation([0, 1], 1.0, 8).compute_for_analysis(la)
    with pytest.raises(NotImplementedError):
        RadialDistribution(1.0, 8).compute_for_analysis(la)
