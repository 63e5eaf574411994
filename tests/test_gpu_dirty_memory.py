"""GPU: every entry point on device memory that arrives dirty.

``SITATOR_DEBUG_FILL=<two hex digits>`` (sitator_amd/csrc/debug_fill.h) makes the library fill every buffer ``sit_dmalloc`` hands out,
the bytes of the context's scratch a call is about to use and every raw allocation with that byte first.  A probe below is one
family's smallest rich case, built from that family's own helpers and compared the way that family's own test compares it; it makes
its calls TWICE on one context and returns both results as named arrays.  Per fill a probe asserts

(a) the family's own comparison with its restatement, oracle or golden (inside the probe: the same ``array_equal`` / ``tobytes`` /
    tolerance, no new one),
(b) where the family's own test demands the same bytes of two calls: the filled results are the bytes of the same probe with the
    knob unset,
(c) the second call on the same context gives the bytes of the first - its scratch now holds the fill, not the first call's answer.

``ff`` is NaN as a float, -1 as an integer and the cleared state of several tables; ``7b`` is a finite 1e286 / 1e36 and a large
positive integer, never a sentinel and visible in any sum.

The entry points each probe reaches (``test_every_entry_point_that_allocates_has_a_probe`` compares this list with include/*.h):

PROBES = {
 "landmark":      sit_create sit_destroy sit_site_vertex_distances sit_set_basis sit_set_frames sit_upload_fill_fit sit_fill
                  sit_fit_reset sit_fit_push_stored_rows sit_fit_get_state sit_set_centers sit_predict sit_get_assignments
                  sit_get_rows_dense sit_gram sit_best_match sit_best_match_groups sit_weighted_row_sums sit_site_anchors
                  sit_site_sums sit_check_occupancy sit_jump_list
 "classifier":    sit_set_rows_dense sit_fit_push_dense_rows sit_fit_set_state sit_fit_get_state sit_count_zero_rows sit_predict
 "fill_assign":   sit_fill sit_fill_result sit_predict sit_set_centers sit_get_assignments sit_get_rows_dense
 "dynamic_map":   sit_fill sit_get_rows_dense sit_get_rows_sparse sit_static_seen
 "candidates":    sit_candidate_table sit_set_basis sit_fill
 "labels":        sit_set_assignments sit_jump_list sit_jump_sources sit_jump_analysis sit_assign_last_known sit_running_mode
                  sit_site_counts sit_label_ends sit_replace_unassigned sit_unknown_runs sit_replace_closer
 "merge":         sit_cooccupancy sit_jump_analysis sit_set_assignments sit_distances
 "group":         sit_group_by_site sit_grouped_fetch sit_grouped_bucket_averages sit_grouped_recenter_step sit_site_counts
 "hull":          sit_grouped_hull_volumes sit_grouped_work_fetch sit_grouped_recenter_step sit_group_info
 "clamp":         sit_clamp_trajectory sit_frames_device_ptr sit_set_frames_device
 "recenter":      sit_recenter sit_recenter_resident
 "spectrum":      sit_speed_spectrum
 "msd":           sit_msd
 "vanhove":       sit_vanhove
 "scattering":    sit_scattering
 "density":       sit_density sit_density_peaks
 "percolation":   sit_percolation_components sit_percolation_levels
 "landscape":     sit_landscape_energies
 "barrier":       sit_barrier_energies
 "pathways":      sit_pathway_components sit_min_image
 "voronoi":       sit_voronoi_nodes
 "coordenv":      sit_coordination_environments
 "soap":          sit_soap_vectors sit_soap_site_averages
 "pca":           sit_pca_covariance sit_pca_project
 "dpc":           sit_dpc_graph sit_dpc_assign
 "pbc":           sit_wrap_points sit_distances sit_average
 "shards":        sit_gram_limbs sit_weighted_row_sums_limbs sit_assign_last_known sit_running_mode sit_cooccupancy
 "comm":          sit_comm_create sit_comm_destroy sit_comm_allreduce sit_comm_allgather sit_comm_broadcast sit_comm_barrier
                  sit_comm_info sit_comm_attach sit_gram_limbs sit_weighted_row_sums_limbs
}
"""
import ctypes
import functools
import glob
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOB = "SITATOR_DEBUG_FILL"
FILLS = ("ff", "7b")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry points that neither allocate nor carve: plain getters, setters, plans (pure host arithmetic) and the pool's own switch
EXEMPT = """sit_abi sit_device_count sit_last_message sit_timers sit_info sit_synchronize sit_release_cached_memory
sit_comm_unique_id sit_row_width
sit_group_plan sit_hull_plan sit_barrier_plan sit_soap_plan sit_dpc_plan sit_voronoi_plan sit_coordenv_plan sit_vanhove_plan
sit_scattering_plan sit_density_plan sit_percolation_plan sit_landscape_plan""".split()


# ---- the runner -------------------------------------------------------------------------------------------------------

def _bytes(v):
    if v is None:
        return None
    a = np.ascontiguousarray(v)
    return (a.dtype.str, a.shape, a.tobytes())


def assert_same_bytes(got, want, what):
    assert sorted(got) == sorted(want), what
    for name in want:
        assert _bytes(got[name]) == _bytes(want[name]), "%s: %s" % (what, name)


_CLEAN = {}


def run_dirty(probe, fill, mp, same_bytes_as_clean=True):
    """``probe(mp) -> (first, second)``: two rounds of the same calls on one context, each a dict of named arrays, each already
    held against the family's reference.  Once with the knob unset (kept for the other fill), then under ``fill``."""
    name = probe.__name__
    if name not in _CLEAN:
        mp.delenv(KNOB, raising=False)
        clean = probe(mp)
        assert_same_bytes(clean[1], clean[0], "%s, knob unset, second call" % name)
        _CLEAN[name] = clean[0]
    mp.setenv(KNOB, fill)
    first, second = probe(mp)
    assert_same_bytes(second, first, "%s under %s: the second call on the context" % (name, fill))          # (c)
    if same_bytes_as_clean:
        assert_same_bytes(first, _CLEAN[name], "%s under %s against the knob unset" % (name, fill))          # (b)


def twice(make_context, calls):
    with make_context() as ctx:
        return calls(ctx), calls(ctx)


def plain_context(cell):
    from sitator_amd import _lib
    return _lib.HipContext(np.asarray(cell, dtype=np.float64))


# ---- 0. the knob reaches the device -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", FILLS)
def test_a_buffer_nobody_wrote_holds_the_fill(fill, monkeypatch):
    """``sit_set_frames`` without a host array allocates the frames and uploads nothing: read back by the HIP runtime itself they
    are the fill, byte for byte (and whatever they are with the knob unset, the call is the same)."""
    from sitator_amd import _lib
    from tests.test_gpu_msd import Context
    from tests.test_gpu_vibfreq import resident_frames
    monkeypatch.setenv(KNOB, fill)
    frames = np.zeros((3, 140, 3))
    with Context(frames=frames) as ctx:
        S = 140 - ctx.M
        sidx, midx = np.arange(S, dtype=np.int64), np.arange(S, 140, dtype=np.int64)
        # a longer trajectory: the frames' buffer is taken anew
        ctx.F = 5
        ctx._check(ctx.lib.sit_set_frames(ctx._h, None, 5, 140, _lib._i(sidx), S, _lib._i(midx), len(midx), 0))
        got = resident_frames(ctx)
    assert got.shape == (5, 140, 3) and set(got.tobytes()) == {int(fill, 16)}


# ---- 1. the frame-series operators --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _spectrum_case(n):
    from tests import vibfreq_ref as V
    traj = V.random_walk(n + 1, 3, seed=n)
    return traj, V.restatement(traj, slice(None))


def probe_spectrum(mp):
    """n = 257 in one pass and n = 33 with three-bit passes (the three-pass chain), spectrum and speeds fetched."""
    from tests.test_gpu_vibfreq import Context, check_against_numpy, host_call

    def calls(ctx):
        out = {}
        for n, bits in ((257, None), (33, "3")):
            if bits:
                mp.setenv("SITATOR_SPECTRUM_STAGE_BITS", bits)
            else:
                mp.delenv("SITATOR_SPECTRUM_STAGE_BITS", raising=False)
            traj, ref = _spectrum_case(n)
            got = host_call(ctx, traj, slice(None))
            check_against_numpy(ref, *got)
            out.update({"%d/%s" % (n, k): v for k, v in zip(("avg", "power", "spectrum", "speeds"), got)})
        mp.delenv("SITATOR_SPECTRUM_STAGE_BITS", raising=False)
        return out
    return twice(Context, calls)


@functools.lru_cache(maxsize=None)
def _msd_case():
    from tests import msd_ref as R
    from tests.test_gpu_msd import DRIFT, wrapped_walk
    cell, F = R.HEX, 100
    wrapped, _, ref = wrapped_walk(F, 4, 51, cell, drift=DRIFT)
    y = R.series(wrapped, cell)
    return cell, F, wrapped, ref, y, R.collective_series(y)


def probe_msd(mp):
    """F = 100, four atoms: the direct lags with the fourth moment, all lags through three-bit passes (three passes at this
    length), the collective series on both paths, the images."""
    from tests import msd_ref as R
    from tests.test_gpu_msd import Context, check_all_lags, check_direct
    cell, F, wrapped, ref, y, Y = _msd_case()
    lags = [0, 1, 2, F // 2, F - 2, F - 1]

    def calls(ctx):
        mp.setenv("SITATOR_SPECTRUM_STAGE_BITS", "3")
        msd, _, coll, images, res = ctx.msd(positions=wrapped, max_lag=F - 1, collective=True, images=True)
        mp.delenv("SITATOR_SPECTRUM_STAGE_BITS", raising=False)
        plain = ctx.msd(positions=wrapped, max_lag=F - 1)[0]
        d_msd, d_r4, d_coll, _, d_res = ctx.msd(positions=wrapped, lags=lags, r4=True, collective=True)
        check_all_lags(y, msd)
        check_all_lags(y, plain)
        check_all_lags(Y, coll[None] * 4.0, "collective ")
        check_direct(y, lags, d_msd, d_r4)
        check_direct(Y, lags, d_coll[None] * 4.0, np.zeros((1, len(lags))) + np.asarray(R.msd_direct(Y, lags)[1], dtype=np.float64))
        assert np.array_equal(images, ref[1]) and res == ref[2] == d_res
        return dict(msd=msd, plain=plain, coll=coll, images=images, res=np.float64(res), d_msd=d_msd, d_r4=d_r4, d_coll=d_coll)
    return twice(lambda: Context(cell), calls)


@functools.lru_cache(maxsize=None)
def _vanhove_case():
    """The family's ``crowd``: F = 97, two lists out of 140 atoms, both parts rich (asserted from the restatement alone)."""
    from tests import msd_ref as R
    from tests import test_gpu_vanhove as T
    from tests.test_gpu_msd import Context, DRIFT, wrapped_walk
    cell = Context.resident_cell()
    assert np.all(R.heights(cell) >= 3.0)
    x, _, _ = wrapped_walk(97, 140, 33, cell, drift=DRIFT)
    a, b = np.array([3, 17, 40, 41, 99]), np.concatenate([np.arange(50, 110), np.arange(120, 130)])
    lags, r_max, n_bins = T.lags_of(97, (5, 20, 50)), T.r_limit(cell, 0.15), 16
    sc, dc, res = T.reference(x, cell, a, b, False, lags, 1, r_max, n_bins)
    assert T.rich(sc) and T.rich(dc)
    T.check_row_sums(sc, dc, 97, lags, 1, len(a), len(b), False)
    return dict(cell=cell, x=x, a=a, b=b, lags=lags, r_max=r_max, n_bins=n_bins, sc=sc, dc=dc, res=res)


def probe_vanhove(mp):
    """Both parts with every frame held, with a workspace of five frames (windows, a lag at a time, one atom's series at a time)
    and with four histogram copies a workgroup."""
    from tests import test_gpu_vanhove as T
    from tests.test_gpu_msd import Context
    c = _vanhove_case()
    frame = (len(c["a"]) + len(c["b"])) * 24

    def calls(ctx):
        out = {}
        for name, kw, copies in (("whole", {}, None), ("five", dict(workspace_bytes=512 + 5 * frame), None), ("copies", {}, "4")):
            if copies:
                mp.setenv("SITATOR_VANHOVE_HIST_COPIES", copies)
            got = T.device(ctx, c["x"], c["a"], c["b"], False, c["lags"], 1, c["r_max"], c["n_bins"], **kw)
            mp.delenv("SITATOR_VANHOVE_HIST_COPIES", raising=False)
            assert got[0].dtype == got[1].dtype == np.uint64
            assert np.array_equal(got[0], c["sc"]) and np.array_equal(got[1], c["dc"]) and got[2] == c["res"], name
            out[name + "/self"], out[name + "/distinct"], out[name + "/res"] = got[0], got[1], np.float64(got[2])
        return out
    return twice(lambda: Context(c["cell"]), calls)


@functools.lru_cache(maxsize=None)
def _scattering_case():
    from tests import msd_ref as R
    from tests import scattering_ref as S
    from tests import test_gpu_scattering as T
    from tests.test_gpu_msd import DRIFT, wrapped_walk
    cell_name, F, n_a, n_b, stride, extra, n_random, most = T.CASES["past_a_block_by_one"]
    cell = R.CELLS[cell_name]
    x, _, _ = wrapped_walk(F, n_a + n_b, 200 + F + n_a, cell, drift=DRIFT)
    a, b = np.arange(n_a), n_a + np.arange(n_b)
    q, lags = T.q_list(F + n_a, n_random, most), T.lags_of(F, extra)
    ss, cs = S.sums(x, cell, a, b, False, q, lags, stride)
    origins = np.array([S.n_origins(F, int(t), stride) for t in lags])
    assert np.all(ss[lags == 0] == origins[0] * n_a) and np.all(np.abs(cs[:, 0] - origins * n_a * len(b)) < 1e-6 * origins * n_a * len(b))
    return cell, x, a, b, q, lags, stride, ss, cs


def probe_scattering(mp):
    """The family's ``past_a_block_by_one``: two lists, a block of origins and one more, both parts, and the smallest workspace."""
    from tests import scattering_ref as S
    from tests import test_gpu_scattering as T
    from tests.test_gpu_msd import Context
    cell, x, a, b, q, lags, stride, ss, cs = _scattering_case()

    def calls(ctx):
        got = T.device(ctx, x, a, b, False, q, lags, stride)
        only_c = T.device(ctx, x, a, b, False, q, lags, stride, self_part=False)
        assert T.same_bytes(got[0], ss) and T.same_bytes(got[1], cs) and only_c[0] is None and T.same_bytes(only_c[1], cs)
        return {"self": got[0], "coherent": got[1], "coherent_alone": only_c[1]}
    return twice(lambda: Context(cell), calls)


@functools.lru_cache(maxsize=None)
def _density_case():
    from tests import density_ref as R
    from tests import test_gpu_density as T
    from tests.test_gpu_msd import Context
    cell = Context.resident_cell()
    x = T.walk(150, 30, 35, cell)
    atoms, grid = np.array([3, 17, 20, 21, 29, 0, 1]), (17, 16, 33)
    counts = R.counts(x, cell, atoms, grid)[0]
    box = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    w = np.random.default_rng(4).normal(size=27)
    far = (np.array([[8, 7, 0], [-8, -7, 3], [0, 1, 0], [0, 0, -16]]), np.array([0.5, 0.25, -2.0, 1e-3]))
    assert R.plan(150, 30, 7, grid, n_taps=4, halo3=(8, 7, 16))["smooth_lds"] == 0          # this stencil reads memory
    rng = np.random.default_rng(9)                                  # the family's largest peak grids: many ties, and a normal field
    peak_grids = [(rng.integers(0, 4, size=(17, 16, 5)).astype(float), 0.5), (rng.normal(size=(17, 16, 5)), 0.0)]
    peaks = [R.peaks(g, thr) for g, thr in peak_grids]
    assert all(len(p) >= 3 for p in peaks)
    return dict(cell=cell, x=x, atoms=atoms, grid=grid, counts=counts, box=(box, w), far=far, smooth_box=R.smooth(counts, box, w),
                smooth_far=R.smooth(counts, *far), peak_grids=peak_grids, peaks=peaks)


def probe_density(mp):
    """The family's ``crowd``: the counts in both forms, smoothed over the LDS tile (27 signed taps) and from memory (taps beyond the
    tile), and the peaks of a smoothed grid."""
    from sitator_amd import _lib_density
    from tests import test_gpu_density as T
    from tests.test_gpu_msd import Context
    c = _density_case()

    def calls(ctx):
        out = {}
        for form in (1, 2):
            for name in ("box", "far"):
                taps, w = c[name]
                got = T.device(ctx, c["x"], c["atoms"], c["grid"], taps=taps, weights=w, form=form)
                assert T.same_bytes(got[0], c["counts"]) and T.same_bytes(got[1], c["smooth_" + name]), (form, name)
                out["%d/%s/counts" % (form, name)], out["%d/%s/smooth" % (form, name)] = got[0], got[1]
        for i, ((g, thr), want) in enumerate(zip(c["peak_grids"], c["peaks"])):
            peaks = _lib_density.density_peaks(ctx, g, thr)
            assert peaks.dtype == np.int64 and np.array_equal(peaks, want)
            out["peaks/%d" % i] = peaks
        return out
    return twice(lambda: Context(c["cell"]), calls)


@functools.lru_cache(maxsize=None)
def _percolation_case():
    from tests import percolation_ref as R
    shape = (17, 16, 33)
    field = np.random.default_rng(100 + 26 + shape[0]).random(shape)
    level = 1.0 - 0.0976                                             # at the threshold of 26 neighbours (the family's THRESHOLD)
    comp = R.components(field, level, 26)
    assert len(comp[1]) >= 3                                         # several components, so a stale root or size shows
    lev = R.levels(field, 26)
    return field, level, comp, lev


def probe_percolation(mp):
    """A random field on 17 x 16 x 33 (partial tiles on every axis) at the threshold of 26 neighbours: the components in both forms,
    the three levels."""
    from tests import msd_ref as M
    from tests import test_gpu_percolation as T
    from tests.test_gpu_msd import Context
    field, level, comp, (exp_t, exp_r) = _percolation_case()

    def calls(ctx):
        out = {}
        T.check_components(ctx, field, level, 26, exp=comp, forms=(1, 2))
        for form in (1, 2):
            labels, rec, _ = T.device_components(ctx, field, level, 26, form)
            t, r, info = T.device_levels(ctx, field, 26, form)
            assert t.tobytes() == exp_t.tobytes() and T.same_bytes(r, exp_r) and 0 < info[0] <= 3 * 64
            out.update({"%d/labels" % form: labels, "%d/records" % form: rec, "%d/levels" % form: t, "%d/ranks" % form: r})
        return out
    return twice(lambda: Context(M.ORTHO), calls)


@functools.lru_cache(maxsize=None)
def _landscape_case():
    from tests import barrier_ref as BR
    from tests import landscape_ref as LR
    from tests import test_gpu_landscape as T
    cell, grid, S = BR.SMALL_TRICLINIC, (2, 3, 5), 5                 # tens of images of every atom, a list over several chunks
    rc = 2.2 * BR.heights(cell).min()
    pos, eps, sigma = T.lattice(cell, S, 100 + S + grid[2])
    vox = T.sample(grid)
    return cell, grid, rc, pos, eps, sigma, vox, LR.energies(cell, pos, eps, sigma, rc, grid, vox)


def probe_landscape(mp):
    """The family's SMALL_TRICLINIC, 2 x 3 x 5, five atoms, a cutoff of 2.2 heights: the direct and the tiled form, every voxel."""
    from tests import test_gpu_landscape as T
    cell, grid, rc, pos, eps, sigma, vox, want = _landscape_case()

    def calls(ctx):
        got, tiled = T.check_forms(ctx, pos, eps, sigma, rc, grid)
        assert 10 * len(vox) >= got.size and got.reshape(-1)[vox].tobytes() == want.tobytes() and tiled[2] >= 2
        return dict(energies=got)
    return twice(lambda: T.context(cell), calls)


@pytest.mark.parametrize("fill", FILLS)
def test_spectrum(fill, monkeypatch):
    run_dirty(probe_spectrum, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_msd(fill, monkeypatch):
    run_dirty(probe_msd, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_vanhove(fill, monkeypatch):
    run_dirty(probe_vanhove, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_scattering(fill, monkeypatch):
    run_dirty(probe_scattering, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_density(fill, monkeypatch):
    run_dirty(probe_density, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_percolation(fill, monkeypatch):
    run_dirty(probe_percolation, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_landscape(fill, monkeypatch):
    run_dirty(probe_landscape, fill, monkeypatch)


# ---- 2. LandmarkAnalysis.run, dynamic mapping, the pruning tables -----------------------------------------------------------

# (golden case, tag, environment of the run): the fast and the serial fit, the pipelined upload + fill + fit in chunks of 500
# frames, both assignment plugins, and the three ways to the site centres (real-weighted, real-unweighted, representative landmark)
LANDMARK_RUNS = [("c1_hex_scgrid", "dotprod", {"SITATOR_PIPELINE": "0"}),
                 ("c1_hex_scgrid", "dotprod", {"SITATOR_PIPELINE": "0", "SITATOR_FIT": "s"}),
                 ("c1_hex_scgrid", "dotprod", {"SITATOR_PIPELINE": "1", "SITATOR_PIPE_CHUNK_FRAMES": "500"}),
                 ("c1_hex_scgrid", "mcl", {"SITATOR_PIPELINE": "0"}),
                 ("c1_hex_scgrid", "mcl", {"SITATOR_PIPELINE": "0", "SITATOR_FIT": "s"}),
                 ("c1_hex_scgrid", "mcl_replmk", {"SITATOR_PIPELINE": "0"}),
                 ("c1_variants", "unweighted", {"SITATOR_PIPELINE": "0"})]


def _landmark_run(name, tag, env, mp):
    """One ``LandmarkAnalysis.run`` on a golden case, held against the golden as tests/test_gpu_parity.py holds it."""
    from sitator_amd import LandmarkAnalysis
    from tests import golden_util as G
    from tests import test_gpu_parity as T
    c = T.case(name)
    exp = c.out(tag)
    with mp.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        la = LandmarkAnalysis(verbose=False, **c.kwargs(tag))
        st = la.run(T.make_sn(c), c.frames)
        assert bool(getattr(la, "_pipelined", False)) == (env.get("SITATOR_PIPELINE") == "1")
        lvecs = np.array(la.landmark_vectors)
        jumps = np.array(list(st.jumps()), dtype=np.int64).reshape(-1, 4)
        jumps_u = np.array(list(st.jumps(unknown_as_jump=True)), dtype=np.int64).reshape(-1, 4)
    T.assert_lvecs(lvecs, exp["lvecs"])
    assert la.n_all_zero_lvecs == int(exp["n_all_zero_lvecs"])
    assert st.traj.dtype == np.int64 and np.array_equal(st.traj, exp["labels"]), "site indices must be bit-identical"
    counts = np.bincount(st.traj[st.traj >= 0], minlength=st.site_network.n_sites)
    assert np.array_equal(counts, exp["counts"])
    m = exp["labels"] >= 0
    np.testing.assert_allclose(st.confidences[m], exp["confs"][m], rtol=T.RTOL)
    np.testing.assert_allclose(st.site_network.centers, exp["site_centers"], rtol=T.RTOL, atol=1e-8)
    assert la.n_multiple_assignments == int(exp["n_multiple_assignments"])
    assert la.avg_mobile_per_site == pytest.approx(float(exp["avg_mobile_per_site"]), rel=1e-12)
    assert [tuple(r) for r in jumps.tolist()] == [tuple(r) for r in exp["jumps"]]
    assert [tuple(r) for r in jumps_u.tolist()] == [tuple(r) for r in exp["jumps_unknown"]]
    if "site_vertices" in exp:
        assert [sorted(v) for v in st.site_network.vertices] == G.vertices_of(exp["site_vertices"])
    return dict(labels=st.traj, confs=st.confidences, centers=np.asarray(st.site_network.centers), lvecs=lvecs, jumps=jumps,
                jumps_unknown=jumps_u, n_multi=np.int64(la.n_multiple_assignments), avg=np.float64(la.avg_mobile_per_site))


def probe_landmark(mp):
    """``LandmarkAnalysis.run`` is one-shot and makes its context itself: the two rounds are two runs (the second finds what the
    first gave back to the pool and to the driver)."""
    def round_():
        out = {}
        for name, tag, env in LANDMARK_RUNS:
            key = "%s/%s/%s" % (name, tag, ",".join("%s=%s" % kv for kv in sorted(env.items())))
            out.update({"%s/%s" % (key, k): v for k, v in _landmark_run(name, tag, env, mp).items()})
        return out
    return round_(), round_()


@functools.lru_cache(maxsize=None)
def _classifier_case():
    from tests import golden_util as G
    return G.load("dotprod_known_answers")


def probe_classifier(mp):
    """``DotProdClassifier`` on a host matrix (tests/test_gpu_parity.py ``test_dotprod_classifier_against_reference``): dense rows
    set and pushed through the fit, a fit state set from the host, predict with and without normalisation, the zero-row count."""
    import json
    from sitator_amd import DotProdClassifier
    from tests import test_gpu_parity as T
    z = _classifier_case()
    X = z["X"]

    def round_():
        out = {}
        for tag, thr in (("t045", 0.45), ("t090", 0.9)):
            clf = DotProdClassifier(threshold=thr, min_samples=1)
            clf.fit_centers(X[z[tag + "/fit_input_rows"]])
            assert clf.cluster_centers.shape == z[tag + "/centers"].shape
            np.testing.assert_allclose(clf.cluster_centers, z[tag + "/centers"], rtol=1e-9, atol=1e-14)
            out[tag + "/centers"] = np.array(clf.cluster_centers)
        for tag in ("fp_int", "fp_float", "fp_raw"):
            p = json.loads(str(z[tag + "/params"]))
            clf = DotProdClassifier(threshold=p["threshold"], min_samples=p["min_samples"])
            lab, conf, info = clf.fit_predict(X, predict_threshold=p["predict_threshold"], predict_normed=p["normed"], return_info=True,
                                              verbose=False)
            assert np.array_equal(lab, z[tag + "/labels"]) and np.array_equal(clf.cluster_counts, z[tag + "/counts"])
            assert np.array_equal(info["kept_clusters_mask"], z[tag + "/mask"])
            m = lab >= 0
            np.testing.assert_allclose(conf[m], z[tag + "/confs"][m], rtol=T.RTOL)
            np.testing.assert_allclose(clf.cluster_centers, z[tag + "/centers"], rtol=1e-9, atol=1e-14)
            out.update({tag + "/labels": lab, tag + "/confs": conf, tag + "/centers": np.array(clf.cluster_centers),
                        tag + "/counts": np.asarray(clf.cluster_counts)})
        clf = DotProdClassifier(threshold=0.45, min_samples=1)
        clf.fit_centers(z["quirk/X"])
        np.testing.assert_allclose(clf.cluster_centers, z["quirk/centers"], rtol=1e-9, atol=1e-14)
        out["quirk/centers"] = np.array(clf.cluster_centers)
        return out
    return round_(), round_()


def probe_dynamic_map(mp):
    """C2 (S = 512: the strided loops of k_lattice_map run twice) with a fresh permutation of the statics in every frame, and the
    frame with an atom nobody saw (``static_seen``); the sparse rows are the dense ones."""
    from sitator_amd import _lib
    from tests import dynmap_ref as R
    from tests import test_gpu_dynamic_mapping as T
    c = R.case("C2", 64, 12, "all")
    (exp, nz_exp), (plain, nz_plain) = R.references("C2", 64, 12, "all")
    assert nz_exp == nz_plain and np.array_equal(exp, plain), "the two references must be one"
    cu, pf, perms, a = R.unassigned_case("C2", 64, 8)
    exp_u, nz_u = R.oracle_fill(cu, pf, dynamic_lattice_mapping=True, static_movement_threshold=5.0, relaxed_lattice_checks=True)

    def make(case, frames, static_thr):
        ctx = _lib.HipContext(case.cell)
        try:
            ctx.set_basis(case.ref_static, case.verts, case.vcd, 1.5, 30, static_thr)
            ctx.set_frames(frames, case.sidx, case.midx)
        except Exception:
            ctx.close()
            raise
        return ctx

    def calls(ctx):
        got, nz = T._fill(ctx)
        assert ctx.info()["fill_kernel"] == 3
        T._assert_oracle_rows(got, nz, exp, nz_exp)
        nnz, idx, val = ctx.rows_sparse()
        dense = np.zeros_like(got)
        for e in range(idx.shape[0]):
            live = nnz > e
            dense[np.nonzero(live)[0], idx[e][live]] = val[e][live]
        assert np.array_equal(dense, got)
        return dict(rows=got, nz=np.int64(nz), nnz=nnz)

    def calls_unassigned(ctx):
        rc, _, err = ctx.fill(dynamic_lattice_mapping=True, check_for_zeros=False)
        assert rc == _lib.E_STATIC_UNASSIGNED and err.frame == 4
        seen = ctx.static_seen(4)
        assert perms[4][np.flatnonzero(seen == 0)].tolist() == [a]
        got, nz = T._fill(ctx, relaxed_lattice_checks=True)
        T._assert_oracle_rows(got, nz, exp_u, nz_u)
        return dict(seen=seen, rows=got)

    first, second = twice(lambda: make(c, c.pf, 1.0), calls)
    f2, s2 = twice(lambda: make(cu, pf, 5.0), calls_unassigned)
    first.update({"unassigned/" + k: v for k, v in f2.items()})
    second.update({"unassigned/" + k: v for k, v in s2.items()})
    return first, second


@functools.lru_cache(maxsize=None)
def _assign_case(cfg, M, F):
    """The trajectory of the family's ``test_fused_assign_equals_fill_then_predict`` (seed 5) and the oracle's centres of its rows."""
    from oracle import oracle
    from sitator_amd import synth
    from tests.test_gpu_kernels import _setup
    oracle.lib()
    host = synth.config_host(cfg)
    knob = os.environ.pop(KNOB, None)                                # the reference's input is made without the fill
    try:
        ctx, frames, sm, mm, ref = _setup(host, M, F, seed=5)
        try:
            assert ctx.fill()[0] == 0
            X = ctx.rows_dense()
        finally:
            ctx.close()
    finally:
        if knob is not None:
            os.environ[KNOB] = knob
    centers = oracle.fit_centers(X, 0.45)
    with np.errstate(divide="ignore", invalid="ignore"):
        normed = centers / np.linalg.norm(centers, axis=1)[:, None]
    lab_o, conf_o = oracle.predict(X, centers, 0.8, True)
    assert (lab_o >= 0).any() and (cfg != "C5" or (X != 0).sum(axis=1).max() > 4)          # rows are assigned; C5 has wide rows
    return normed, lab_o, conf_o


def probe_fill_assign(mp):
    """``sit_fill`` with ``assign`` on C2 (narrow rows) and C5 (mostly wide rows): the assignment as kernels of its own behind the fill
    (SITATOR_FUSE=0: the segment lengths are zeroed before the fill kernel and found again by the assignment's carve), inside
    k_fill3 with the rows stored and not, the library's own choice of the form, and deferred passes collected by ``fill_result`` -
    each against fill, then predict, and against the oracle."""
    from sitator_amd import synth
    from tests.test_gpu_kernels import _setup
    first, second = {}, {}
    for cfg, M, F in (("C2", 64, 300), ("C5", 160, 120)):
        normed, lab_o, conf_o = _assign_case(cfg, M, F)
        holder = {}

        class Made(object):
            def __enter__(self):
                holder["ctx"] = _setup(synth.config_host(cfg), M, F, seed=5)[0]
                return holder["ctx"]

            def __exit__(self, *exc):
                holder["ctx"].close()

        def calls(ctx):
            out = {}
            mp.delenv("SITATOR_FUSE", raising=False)
            assert ctx.fill()[0] == 0
            X = ctx.rows_dense()
            ctx.set_centers(normed, True)
            lab_a, conf_a, cnt_a = ctx.predict(0.8)
            assert np.array_equal(lab_o, lab_a)
            m = lab_o >= 0
            np.testing.assert_allclose(conf_a[m], conf_o[m], rtol=1e-6)
            out.update(rows=X, labels=lab_a, confs=conf_a, counts=cnt_a)
            for fuse, store, defer in (("0", True, False), ("1", True, False), ("1", False, False), (None, True, False),
                                       ("0", True, True), ("1", False, True), (None, False, True)):
                if fuse is None:
                    mp.delenv("SITATOR_FUSE", raising=False)
                else:
                    mp.setenv("SITATOR_FUSE", fuse)
                if defer:
                    for _ in range(3):                                # three passes in flight, then collected
                        rc, nz, _ = ctx.fill(assign=True, predict_threshold=0.8, store_rows=store, defer=True)
                        assert rc == 0 and nz == -1
                    rc, nz, _ = ctx.fill_result()
                    assert rc == 0 and nz == 0
                else:
                    rc, _, _ = ctx.fill(assign=True, predict_threshold=0.8, store_rows=store)
                    assert rc == 0
                mp.delenv("SITATOR_FUSE", raising=False)
                if fuse is not None:
                    assert ctx.info()["assignment_fused"] == (fuse == "1"), "the requested form of the pass did not run"
                lab_b, conf_b, cnt_b = ctx.assignments()
                key = "%s/%d/%d" % (fuse, store, defer)
                assert np.array_equal(lab_a, lab_b) and np.array_equal(conf_a, conf_b) and np.array_equal(cnt_a, cnt_b), key
                if store:
                    assert np.array_equal(ctx.rows_dense(), X), key
                out.update({key + "/labels": lab_b, key + "/confs": conf_b, key + "/counts": cnt_b})
            return out
        a, b = twice(Made, calls)
        first.update({cfg + "/" + k: v for k, v in a.items()})
        second.update({cfg + "/" + k: v for k, v in b.items()})
    return first, second



_CAND_PROBE = {}


def probe_candidates(mp):
    """The loose table after ``set_basis`` and the tight table after a fill of 32 jittered frames, on the ragged basis, against the
    exhaustive reference and the host probe's table; the second round sets the basis again on the same context."""
    from tests import test_candidates_plan as P
    from tests import test_gpu_candidates as T
    case = P.cases()["ragged"]
    host_probe = _CAND_PROBE["probe"]
    rng = np.random.default_rng(17)
    frames = np.empty((32, case.S + 1, 3))
    frames[:, :-1] = case.ref_static + rng.normal(scale=0.01, size=(32, case.S, 3))
    frames[:, -1] = case.centers[0] + rng.normal(scale=0.05, size=(32, 3))

    def calls(ctx):
        ctx.set_basis(case.ref_static, case.verts, case.vcd, P.MIDPOINT, P.STEEPNESS, P.STATIC_THR)
        with pytest.raises(ValueError, match="no tight table"):
            ctx.candidate_table(1)
        info = ctx.info()
        loose = ctx.candidate_table(0)
        assert loose["displacement"] == P.STATIC_THR
        T._check_device_table(case, host_probe, loose, info["row_width"], info["mean_candidates_loose"], info["grid_loose"], 1.0, "loose")
        ctx.set_frames(frames, np.arange(case.S), np.array([case.S]))
        rc, nz, err = ctx.fill(check_for_zeros=False)
        info = ctx.info()
        assert rc == 0 and info["fill_kernel"] == 3
        tight = ctx.candidate_table(1)
        assert 0.02 < tight["displacement"] < 0.2 and tight["displacement"] == info["delta"]
        T._check_device_table(case, host_probe, tight, info["tight_width"], info["mean_candidates_tight"], info["grid_tight"], 0.5, "tight")
        return {"loose/off": loose["off"], "loose/list": loose["list"], "tight/off": tight["off"], "tight/list": tight["list"],
                "delta": np.float64(tight["displacement"]), "rows": ctx.rows_dense()}
    return twice(lambda: plain_context(case.cell), calls)


@pytest.mark.parametrize("fill", FILLS)
def test_landmark_analysis(fill, monkeypatch):
    run_dirty(probe_landmark, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_classifier(fill, monkeypatch):
    run_dirty(probe_classifier, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_dynamic_map(fill, monkeypatch):
    run_dirty(probe_dynamic_map, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_fill_with_assignment(fill, monkeypatch):
    run_dirty(probe_fill_assign, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_candidates(fill, monkeypatch, tmp_path_factory):
    if "probe" not in _CAND_PROBE:
        from tests import test_candidates_plan as P
        _CAND_PROBE["probe"] = P.build_probe(tmp_path_factory.mktemp("candidates_plan_dirty"))
    run_dirty(probe_candidates, fill, monkeypatch)


# ---- 3. the label kernels ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _label_case():
    """(257, 300) of ``make_labels`` with everything the oracle and the brute force say about it, once."""
    from oracle import oracle
    from tests import replace_ref as R
    from tests import test_gpu_label_kernels as T
    oracle.lib()
    F, M = 257, 300
    lab, K = T.make_labels(F, M, seed=F * 1000 + M)
    missing = T.expected_features(F, M) - T.features(lab, K)
    assert not missing, missing
    c = dict(lab=lab, K=K, F=F, M=M, split=256)
    c["jumps"] = {u: oracle.jumps(lab, unknown_as_jump=u) for u in (False, True)}
    c["ja"] = oracle.jump_analysis(lab, K)
    c["alk"] = oracle.assign_to_last_known_site(lab, 3)
    c["mode"] = {repl: oracle.running_windowed_mode(lab, 3, 4, 3, K, repl) for repl in (True, False)}
    c["halos"] = R.halos(M, seed=3)
    rng = np.random.default_rng(1003)
    c["centers"], c["pos"] = rng.uniform(size=(K, 3)) @ R.CELL, rng.uniform(size=(F, M, 3)) @ R.CELL
    c["closer"], margin = R.closer(oracle, R.CELL, lab, c["centers"], c["pos"], *c["halos"])
    assert margin >= R.MARGIN                                      # no decided frame is a near-tie (checked on the CPU)
    c["runs"] = R.runs(lab, *c["halos"])
    assert len(c["runs"][0]) >= 100 and (c["runs"][0][:, 5] >= 0).sum() >= 100 and (c["runs"][0][:, 5] < 0).any()    # decided runs, and runs that are not
    return c


def probe_labels(mp):
    """Jump list and sources, jump analysis whole and with the halo carried in at frame 256, assign-last-known, the running mode,
    the site counts, the label ends, replace-unassigned in both directions, the unknown runs and replace-closer."""
    from sitator_amd import _lib
    from tests import replace_ref as R
    from tests import test_gpu_label_kernels as T
    c = _label_case()
    lab, K, F, M, s = c["lab"], c["K"], c["F"], c["M"], c["split"]
    before_in, after_in = c["halos"]

    class Three(object):
        """The whole array and its two shards around frame 256."""

        def __enter__(self):
            self.c = [_lib.HipContext(R.CELL) for _ in range(3)]
            return self.c

        def __exit__(self, *exc):
            for x in self.c:
                x.close()

    def upload(ctxs):
        ctxs[0].set_assignments(lab)
        ctxs[1].set_assignments(np.ascontiguousarray(lab[:s]))
        ctxs[2].set_assignments(np.ascontiguousarray(lab[s:]), frame0=s)

    def calls(ctxs):
        whole, c1, c2 = ctxs
        out = {}
        upload(ctxs)
        for u in (False, True):
            rec, last = whole.jump_list(u)
            assert [tuple(r) for r in rec.tolist()] == c["jumps"][u]
            src, last2 = whole.jump_sources(u)
            assert np.array_equal(src, T._sources(c["jumps"][u], F, M)) and np.array_equal(last, last2)
            r1, l1 = c1.jump_list(u)
            r2, l2 = c2.jump_list(u, l1)
            r2[:, 0] += s
            assert [tuple(r) for r in np.concatenate([r1, r2]).tolist()] == c["jumps"][u] and np.array_equal(l2, last)
            out.update({"jumps/%d" % u: rec, "sources/%d" % u: src, "last/%d" % u: last, "jumps2/%d" % u: r2})
        ja = whole.jump_analysis(K)
        exp = c["ja"]
        assert np.array_equal(ja[0], exp["n_ij"]) and np.array_equal(ja[1], exp["time_sum"]) and np.array_equal(ja[2], exp["time_n"])
        assert np.array_equal(ja[3], exp["total_corrected_residences"]) and ja[4] == exp["n_problems"]
        p1 = c1.jump_analysis(K)
        p2 = c2.jump_analysis(K, p1[5], p1[6])
        for i in range(4):
            assert np.array_equal(p1[i] + p2[i], ja[i]), i
        assert p1[4] + p2[4] == ja[4] and np.array_equal(p2[5], ja[5]) and np.array_equal(p2[6], ja[6])
        out.update({"ja/%d" % i: np.asarray(v) for i, v in enumerate(ja)})
        out.update({"ja_halo/%d" % i: np.asarray(v) for i, v in enumerate(p2)})
        t, (mx, avg, re_) = c["alk"]
        labels, fmax, st3, lout, tout = whole.assign_last_known(3)
        assert np.array_equal(labels, t)
        a1 = c1.assign_last_known(3)
        a2 = c2.assign_last_known(3, a1[3], a1[4])
        assert np.array_equal(np.concatenate([a1[0], a2[0]]), t) and np.array_equal(np.concatenate([a1[1], a2[1]]), fmax)
        assert np.array_equal(a1[2] + a2[2], st3) and np.array_equal(a2[3], lout) and np.array_equal(a2[4], tout)
        out.update(alk=labels, alk_fmax=fmax, alk_st=st3, alk_last=lout, alk_time=tout, alk_halo=a2[0])
        upload(ctxs)                                                  # assign-last-known rewrites the resident labels in place
        for repl in (True, False):
            mode, counts = whole.running_mode(3, 4, 3, repl, n_sites=K)
            assert np.array_equal(counts, np.bincount(mode[mode >= 0], minlength=K)) and np.array_equal(mode, c["mode"][repl])
            out["mode/%d" % repl], out["mode_counts/%d" % repl] = mode, counts
        out["site_counts"] = whole.site_counts(K)
        assert np.array_equal(out["site_counts"], np.bincount(lab[lab >= 0], minlength=K))
        first, last = whole.label_ends()
        assert np.array_equal(first, R.ends(lab)[0]) and np.array_equal(last, R.ends(lab)[1])
        out["first"], out["last_known"] = first, last
        for mode in (0, 1):
            got = whole.replace_unassigned(mode, before_in, after_in)
            assert got.dtype == np.int64 and np.array_equal(got, R.replace(lab, mode, before_in, after_in)), mode
            out["replace/%d" % mode] = got
        rec, npos = whole.unknown_runs(before_in, after_in)
        exp_rec, exp_npos = c["runs"]
        assert rec.shape == exp_rec.shape and np.array_equal(rec, exp_rec) and npos == exp_npos
        positions = R.positions_of(rec, c["pos"])
        assert positions.shape == (npos, 3)
        closer = whole.replace_closer(rec, c["centers"], positions)
        assert np.array_equal(closer, c["closer"])
        out["runs"], out["closer"] = rec, closer
        assert np.array_equal(whole.assignments()[0].reshape(lab.shape), lab)           # the resident labels were only read
        return out
    return twice(Three, calls)


def probe_merge(mp):
    """Co-occupancy of the designed (131, 70) labels; ``MergeSitesByThreshold`` with multiple occupancy forbidden and
    ``RemoveUnoccupiedSites`` on the reference's golden."""
    import json
    from sitator_amd import JumpAnalysis, RemoveUnoccupiedSites, SiteTrajectory, _lib
    from tests import cooccupancy_ref as R
    from tests import test_gpu_cooccupancy as T
    lab, K = R.designed_labels(131, 70, seed=5)
    exp = R.brute_cooccupancy(lab, K)
    assert 0.15 < R.off_diagonal_fill(exp) < 0.85
    TG, name = T.TG, "c1_hex_scgrid"

    def operators():
        out = {}
        for variant in ("n1_forbid", "n2_forbid_d40"):
            key = "%s/%s" % (name, variant)
            st = SiteTrajectory(TG.network(name), TG.labels(name).copy())
            JumpAnalysis().run(st)
            err, res = R.run_threshold_variant(st, json.loads(str(TG.z[key + "/params"])))
            assert err == str(TG.z[key + "/error"])
            if not err:
                assert np.array_equal(res.traj, TG.z[key + "/traj"])
                np.testing.assert_allclose(np.asarray(res.site_network.centers), TG.z[key + "/centers"], rtol=1e-6, atol=1e-9)
                out[variant + "/traj"], out[variant + "/centers"] = res.traj, np.asarray(res.site_network.centers)
        st = SiteTrajectory(TG.network(name), TG.labels(name).copy())
        co = st.compute_site_cooccupancy()
        assert co.dtype == np.bool_ and np.array_equal(co, TG.z[name + "/cooccupancy"])
        centers, labels = TG.with_dead_sites(name)
        removed, kept = RemoveUnoccupiedSites().run(SiteTrajectory(TG.network(name, centers), labels), return_kept_sites=True)
        assert np.array_equal(kept[0], TG.z[name + "/rm_a/kept"]) and np.array_equal(removed.traj, TG.z[name + "/rm_a/traj"])
        out.update(co=co, kept=kept[0], removed=removed.traj)
        return out

    def calls(ctx):
        ctx.set_assignments(lab)
        got = ctx.cooccupancy(K)
        assert got.dtype == np.bool_ and got.shape == (K, K) and np.array_equal(got, exp) and np.array_equal(got, got.T)
        out = operators()
        out["designed"] = got
        return out
    return twice(lambda: _lib.HipContext(np.eye(3) * 10.0), calls)


@pytest.mark.parametrize("fill", FILLS)
def test_label_kernels(fill, monkeypatch):
    run_dirty(probe_labels, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_merge_cooccupancy_and_removal(fill, monkeypatch):
    run_dirty(probe_merge, fill, monkeypatch)


# ---- 4. grouping, hulls, the clamped trajectory, recentring -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _group_case():
    from tests import group_ref as GR
    from tests import test_gpu_group as T
    F, M, K = 5, 65, 30                                              # more ions than a wave
    labels, pos, confs = GR.designed(T.CELL, F, M, K, seed=F + M, n_unknown=F * M // 9, consumers=False)
    mobile = GR.layout(M, 3, "interleaved", seed=M)
    midx = np.where(mobile)[0]
    real = GR.embed(mobile, pos, seed=F)
    rec = T.recentring_case([1, 7, 8, 9, 40], seed=2)
    steps = list(GR.recenter_steps(T.CELL, rec[2], rec[3], 8))
    n = 3
    bucket = T.bucket_case(n, seed=n, big=3000)
    bl, bp, bc, off, pts, cf = bucket
    sizes = sorted({len(range(off[s] + i, off[s + 1], n)) for s in range(len(off) - 1) for i in range(n) if off[s + 1] - off[s] > n})
    assert {1, 2, 64, 65}.issubset(sizes) and sizes[-1] >= 3000
    averages = {w: GR.bucket_averages(T.CELL, off, pts, cf, n, w) for w in (True, False)}
    bounds = {w: GR.bucket_bound(T.CELL, off, pts, averages[w][1], n) for w in (True, False)}
    return dict(F=F, M=M, K=K, labels=labels, confs=confs, midx=midx, real=real, want=GR.grouped(labels, K, real, midx, confs), rec=rec,
                steps=steps, n=n, bucket=bucket, averages=averages, bounds=bounds)


def probe_group(mp):
    """Grouping of (5, 65, 30) with everything at once and a frame at a time; the eight recentring steps of sites of 1, 7, 8, 9 and
    40 points; bucket averages of buckets of 1, 2, 64, 65 and 3000 points; ``NAvgsPerSite`` on the reference's golden."""
    from sitator_amd import NAvgsPerSite
    from tests import group_ref as GR
    from tests import test_gpu_group as T
    c = _group_case()
    name = T.GG.names[0]

    def calls(ctx):
        out = {}
        ctx.set_assignments(c["labels"], c["confs"])
        for cap in (0, c["real"].shape[1] * 24):
            off = ctx.group_by_site(c["K"], positions=c["real"], mobile_idx=c["midx"], workspace_bytes=cap)
            T.assert_grouping(ctx, off, c["want"], cap)
            pts, cf, ent = T.fetch_all(ctx, off)
            out.update({"group/%d/offsets" % cap: off, "group/%d/points" % cap: pts, "group/%d/confs" % cap: cf, "group/%d/entries" % cap: ent})
        assert np.array_equal(ctx.site_counts(c["K"]), np.diff(c["want"][0]))
        labels, pos, off, pts = c["rec"]
        ctx.set_assignments(labels)
        assert np.array_equal(ctx.group_by_site(len(off) - 1, positions=pos, mobile_idx=np.arange(1)), off)
        buf = np.empty((int(off[-1]), 3))
        for i, want in enumerate(c["steps"]):
            assert ctx.grouped_recenter_step(i, 8, buf) is buf
            assert np.array_equal(buf, want), i
            out["recenter/%d" % i] = buf.copy()
        assert np.array_equal(T.fetch_all(ctx, off)[0], pts)          # the grouping itself stays
        labels, pos, confs, off, pts, cf = c["bucket"]
        K, n = len(off) - 1, c["n"]
        ctx.set_assignments(labels, confs)
        ctx.group_by_site(K, positions=pos, mobile_idx=np.arange(1))
        for weighted in (True, False):
            want, want_anchor = c["averages"][weighted]
            got, anchor = ctx.grouped_bucket_averages(K, n, weighted)
            assert np.array_equal(anchor, want_anchor) and np.array_equal(np.isnan(got), np.isnan(want))
            m = ~np.isnan(want)
            assert np.all(np.abs(got - want)[m] <= c["bounds"][weighted][m])
            for s in range(K):
                for i in range(n):
                    if want_anchor[s, i] >= 0 and len(range(off[s] + i, off[s + 1], n)) <= 2:
                        assert np.array_equal(got[s, i], want[s, i]), (s, i)
            out["buckets/%d" % weighted], out["anchors/%d" % weighted] = got, anchor
        # the operator on the reference's golden
        cell, Kg = T.GG.get(name, "in_cell"), len(T.GG.get(name, "in_centers"))
        midx = np.where(T.GG.get(name, "in_mobile_mask"))[0]
        goff, _, gpts, gcf = GR.grouped(T.GG.get(name, "in_labels"), Kg, T.GG.get(name, "in_real"), midx, T.GG.get(name, "in_confs"))
        for weighted in (0, 1):
            sn = NAvgsPerSite(2, weighted=bool(weighted)).run(T.GG.trajectory(name, with_confs=bool(weighted)))
            want = T.GG.get(name, "out_navg_w%d_n2_centers" % weighted)
            _, anchors = GR.bucket_averages(cell, goff, gpts, gcf, 2, bool(weighted))
            bound = GR.bucket_bound(cell, goff, gpts, anchors, 2).reshape(-1, 3)
            assert sn.centers.shape == want.shape and np.all(np.abs(np.asarray(sn.centers) - want) <= bound)
            assert np.array_equal(sn.site_types, T.GG.get(name, "out_navg_w%d_n2_types" % weighted))
            out["navg/%d" % weighted] = np.asarray(sn.centers)
        return out
    return twice(T.context, calls)


def probe_hull(mp):
    """The designed grouping ``edges`` (4 to 1025 points a site): working copy, volumes, statuses, facet counts and vertex masks of the
    device hulls; ``SiteVolumes(hulls="device")`` on the reference's golden."""
    from sitator_amd import SiteVolumes
    from tests import hull_ref as HR
    from tests import test_gpu_hull as T
    gname = "edges"
    sites = HR.GROUPINGS[gname]
    K = len(sites)
    want = T.reference(gname)
    name = T.GG.names[0]

    def calls(handle):
        ctx, off, work = handle
        ctx.grouped_recenter_step(0, 1, None)
        assert np.array_equal(ctx.grouped_work_fetch(0, int(off[-1])), work)
        vols, status, nf, mask = ctx.grouped_hull_volumes(K, vertex_mask=True)
        assert np.array_equal(ctx.grouped_work_fetch(0, int(off[-1])), work)                # the kernel only reads
        assert status.dtype == nf.dtype == np.int32 and mask.dtype == np.uint8 and len(mask) == off[-1]
        assert np.array_equal(status, np.zeros(K, dtype=np.int32))
        for s in range(K):
            w = want[s]
            assert w["ref"]["status"] == HR.CLOSED
            got_v = np.nonzero(mask[off[s]:off[s + 1]])[0]
            assert np.array_equal(got_v, w["qhull_vertices"]), s
            assert nf[s] == len(w["ref"]["facets"]), s
            assert abs(HR.Fraction(float(vols[s])) - w["exact"]) <= HR.Fraction(w["bound"]), s
            assert abs(vols[s] - w["qhull_volume"]) <= HR.QHULL_REL_TOL * w["qhull_volume"], s
        out = dict(volumes=vols, status=status, facets=nf, mask=mask)
        for nr in (1, 8):
            st = T.GG.trajectory(name)
            op = SiteVolumes(hulls="device")
            v = op.compute_accessable_volumes(st, n_recenterings=nr)
            ref = T.GG.get(name, "out_access_vol_r%d" % nr)
            assert np.all(np.abs(v - ref) / ref <= HR.QHULL_REL_TOL)
            assert op.last_hull_status == {0: st.site_network.n_sites * nr, 1: 0, 2: 0, 3: 0, 4: 0}      # nothing went to the host
            out["golden/r%d" % nr] = v
        return out
    return twice(lambda: T.grouped(sites), calls)


@functools.lru_cache(maxsize=None)
def _clamp_case():
    from sitator_amd import synth
    from tests import clamp_ref as CR
    from tests import test_gpu_clamped as T
    cell = np.asarray(synth.config_host("C1").cell, dtype=np.float64)
    F, S, M, K = 301, 27, 6, 5
    centers, labels, pos = CR.designed(cell, F, M, K, seed=12, n_unknown=40)
    mobile = np.arange(S + M) >= S
    spos = np.random.default_rng(2).uniform(size=(S + M, 3)) @ cell
    real = CR.embed(mobile, spos, pos, seed=6)
    mask = T.masks(mobile, seed=3)["random"]
    want = {w: CR.clamp(cell, spos, mobile, centers, labels, real, mask, w, True) for w in (False, True)}
    return cell, centers, labels, mobile, spos, real, mask, want


def probe_clamp(mp):
    """The family's resident case (301 frames of 33 atoms: an odd number of doubles a frame) with a random clamp mask: host
    positions, the resident frames, and both again in chunks of seven frames."""
    from sitator_amd import _lib
    from tests import test_gpu_clamped as T
    cell, centers, labels, mobile, spos, real, mask, want = _clamp_case()
    role = T.roles(mobile, mask)
    frame_bytes = len(mobile) * 24

    def calls(ctx):
        out = {}
        ctx.set_assignments(labels)
        for w in (False, True):
            host = ctx.clamp_trajectory(role, spos, centers, w, True, positions=real)
            res = ctx.clamp_trajectory(role, spos, centers, w, True)
            host7 = ctx.clamp_trajectory(role, spos, centers, w, True, positions=real, workspace_bytes=7 * 2 * frame_bytes + 5)
            res7 = ctx.clamp_trajectory(role, spos, centers, w, True, workspace_bytes=7 * frame_bytes + 5)
            for name, got in (("host", host), ("resident", res), ("host7", host7), ("resident7", res7)):
                assert got.dtype == np.float64 and np.array_equal(got, want[w]), (name, w)
                out["%s/%d" % (name, w)] = got
        assert np.array_equal(T.resident_frames(ctx), real)
        assert np.array_equal(ctx.assignments()[0].reshape(labels.shape), labels)
        # a second context adopts the first one's frames where they lie (sit_set_frames_device: only the index arrays are made)
        with T.Context(frames=real[:1]) as other:
            S = int(np.count_nonzero(~mobile))
            sidx, midx = np.arange(S, dtype=np.int64), np.arange(S, len(mobile), dtype=np.int64)
            other._check(other.lib.sit_set_frames_device(other._h, ctx.frames_device_ptr(), len(real), len(mobile), _lib._i(sidx), S,
                                                         _lib._i(midx), len(midx), 0))
            other.F, other.N = len(real), len(real) * len(midx)
            other.set_assignments(labels)
            got = other.clamp_trajectory(role, spos, centers, True, True)
            assert np.array_equal(got, want[True])
            out["adopted"] = got
        return out
    return twice(lambda: T.Context(frames=real), calls)


def probe_recenter(mp):
    """``RecenterTrajectory`` on the reference's golden (positions, velocities, masses) through one context, and the recentring of the
    resident frames as ``LandmarkAnalysis(recenter_masses=...)`` takes it, against recentre-then-run."""
    from sitator_amd import LandmarkAnalysis, RecenterTrajectory, SiteNetwork, Structure, synth
    from tests.test_next_tier import z
    g = z()
    sm = g["rc/static_mask"]
    factors, ones = sm.astype(np.float64), np.ones(len(sm))
    host = synth.config_host("C1b")
    frames, hsm, hmm, ref = synth.make_trajectory(host, 4, 400, seed=31, p_hop=1.0 / 50)
    frames = frames + np.cumsum(np.random.default_rng(3).normal(scale=0.002, size=(len(frames), 1, 3)), axis=0)
    masses = np.random.default_rng(4).uniform(1.0, 40.0, size=frames.shape[1])
    ref_rec = ref[None].copy()
    RecenterTrajectory().run(Structure(ref, host.cell), hsm, ref_rec, masses=masses)
    shift = ref_rec[0, 0] - ref[0]

    def sn_():
        sn = SiteNetwork(Structure(ref_rec[0], host.cell), hsm, hmm)
        sn.centers = np.asarray(host.centers) + shift
        sn.vertices = host.vertices
        return sn

    def calls(ctx):
        p, v, p2 = g["rc/frames"].copy(), g["rc/velocities"].copy(), g["rc/frames"].copy()
        RecenterTrajectory._apply(ctx, p, ones, factors, ctx.cell_centroid)
        RecenterTrajectory._apply(ctx, v, ones, factors, None)
        RecenterTrajectory._apply(ctx, p2, g["rc/masses"].astype(np.float64), factors, ctx.cell_centroid)
        np.testing.assert_allclose(p, g["rc/out_default"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(v, g["rc/out_velocities"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(p2, g["rc/out_masses"], rtol=0, atol=1e-10)
        keep = frames.copy()
        st_a = LandmarkAnalysis(verbose=False, recenter_masses=masses).run(sn_(), frames)
        assert np.array_equal(frames, keep)
        rec = frames.copy()
        RecenterTrajectory().run(Structure(ref, host.cell), hsm, rec, masses=masses)
        st_b = LandmarkAnalysis(verbose=False).run(sn_(), rec)
        assert np.array_equal(st_a.traj, st_b.traj) and np.array_equal(st_a.confidences, st_b.confidences)
        np.testing.assert_allclose(np.asarray(st_a.site_network.centers), np.asarray(st_b.site_network.centers), rtol=0, atol=1e-12)
        return dict(positions=p, velocities=v, weighted=p2, labels=st_a.traj, confs=st_a.confidences, centers=np.asarray(st_a.site_network.centers))
    return twice(lambda: plain_context(g["rc/cell"]), calls)


@pytest.mark.parametrize("fill", FILLS)
def test_group_by_site(fill, monkeypatch):
    run_dirty(probe_group, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_device_hulls(fill, monkeypatch):
    run_dirty(probe_hull, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_clamped_trajectory(fill, monkeypatch):
    run_dirty(probe_clamp, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_recenter(fill, monkeypatch):
    run_dirty(probe_recenter, fill, monkeypatch)


# ---- 5. barrier, pathways, Voronoi nodes, coordination environments, SOAP, PCA, dpc, the PBC surface --------------------------

def probe_barrier(mp):
    """The family's (cubic, S = 65, n = 67, two pairs, atoms outside the cell) and (small triclinic, S = 3, n = 5)."""
    from tests import barrier_ref as BR
    from tests import test_gpu_barrier as T
    specs = [("cubic", 0.45, 65, 67, 2, True), ("small_triclinic", 1.4, 3, 5, 2, True)]
    first, second = {}, {}
    for spec in specs:
        c = T.raw_case(*spec)
        assert c["n_terms"].max() <= 100000 and c["n_terms"].sum() > 0

        def calls(ctx):
            energies, verdict, code = T.call(ctx, c)
            assert energies.shape == c["energies"].shape and np.array_equal(code, c["codes"])
            T.assert_energies_close(energies, c["energies"], c["abs_sums"])
            sure = T.decided(c)
            assert np.array_equal(verdict[sure], c["verdicts"][sure])
            assert np.array_equal(verdict, np.array([BR.verdict(row, c["threshold"]) for row in energies], dtype=np.uint8).reshape(-1, 3))
            return {spec[0] + "/energies": energies, spec[0] + "/verdict": verdict, spec[0] + "/codes": code}
        a, b = twice(lambda: plain_context(c["cell"]), calls)
        first.update(a)
        second.update(b)
    return first, second


def probe_pathways(mp):
    """The random network of 65 sites in the triclinic cell (the family's fuzz): components with the image codes, the minimum
    images of the connected pairs, and the operator."""
    from tests import pathway_ref as PR
    from tests import test_gpu_pathways as T
    cell, K, seed, kw = PR.TRICLINIC, 65, 14, {"connectivity_threshold": 0.004}
    centers, n_ij = PR.random_network(cell, K, seed)
    exp = PR.analyse(cell, centers, n_ij, **kw)
    src, dst = np.nonzero(exp["conn"])
    assert len(src) > K and exp["count"] >= 1
    exp_moved, exp_codes = PR.min_image(cell, centers[src], centers[dst])

    def calls(ctx):
        root, rounds, codes = ctx.pathway_components(exp["conn"], centers, 27, codes=True)
        assert np.array_equal(codes, exp["codes"]) and np.array_equal(PR.ranked(root), exp["labels"])
        moved, mcodes = ctx.min_image(centers[src], centers[dst].copy())
        assert np.array_equal(moved, exp_moved) and np.array_equal(mcodes, exp_codes)
        got = T.run_operator(cell, centers, n_ij, kw)
        T.assert_operator_equal(got, exp)
        return dict(root=root, codes=codes, moved=moved, min_codes=mcodes, site=got["site"], edge=got["edge"], dirs=got["dir_rows"])
    return twice(lambda: plain_context(cell), calls)


def _voronoi_check(name, got):
    from tests import test_gpu_voronoi as T
    from tests import voronoi_ref as VR
    cell, pos = VR.fixture(name)
    ref = VR.stored(name)
    info = got["info"]
    assert np.array_equal(got["status"], ref["status"]) and np.all(got["status"] == VR.OK)
    assert info["rounds"] == ref["rounds"] and info["merge_status"] == VR.OK and info["records"] == ref["records"]
    assert np.array_equal(got["nbr_count"], ref["nbr_count"]) and info["max_neighbours"] == ref["nbr_count"].max()
    assert abs(info["final_radius"] - ref["final_radius"]) <= 1e-12 * ref["final_radius"]
    assert [v.tolist() for v in got["vertices"]] == ref["vertices"]           # the same nodes in the same order
    dc = T.mic_norm(got["centers"] - ref["exact_centers"], cell).max()
    dr = np.abs(got["radii"] - ref["exact_radii"]).max()
    tol = VR.CENTER_TOL if name in VR.GENERIC else T.MU
    assert dc <= tol and dr <= tol


def probe_voronoi(mp):
    """``spread65`` (one atom past a wave) and ``sc_void`` (the driver grows the search radius), in turn on one context - a context
    keeps its last result, so each call computes."""
    from tests import voronoi_ref as VR
    names = ("spread65", "sc_void")

    def round_(ctxs):
        out = {}
        for name in names:
            got = ctxs[name].voronoi_nodes(VR.fixture(name)[1], VR.TAU)
            _voronoi_check(name, got)
            if name == "sc_void":
                assert got["info"]["rounds"] > 1 and max(len(v) for v in got["vertices"]) == 24
            out.update({"%s/%s" % (name, k): got[k] for k in ("centers", "radii", "status", "nbr_count")})
            out[name + "/vertices"] = np.concatenate(got["vertices"])
        return out
    return _two_rounds_on_contexts({n: VR.fixture(n)[0] for n in names}, round_,
                                   lambda ctx, n: ctx.voronoi_nodes(VR.fixture(n)[1], 2.0 * VR.TAU))       # another tolerance: not the kept result


def _two_rounds_on_contexts(cells, round_, other):
    """A context per name; ``round_(contexts)`` twice.  The entry points that come here keep their last result per context, so between
    the rounds ``other(context, name)`` asks every context for something else: the second round computes again."""
    made = {n: plain_context(c) for n, c in cells.items()}
    try:
        first = round_(made)
        for n, ctx in made.items():
            other(ctx, n)
        return first, round_(made)
    finally:
        for ctx in made.values():
            ctx.close()


def probe_coordenv(mp):
    """``fcc_jitter`` and ``sc_void`` (two rounds of the search radius); between the two rounds every context computes another
    request, so the second round is computed too (``size_computed``)."""
    from tests import coordenv_ref as CR
    from tests import test_gpu_coordenv as T
    names = ("fcc_jitter", "sc_void")

    def round_(ctxs):
        out = {}
        for name in names:
            cell, pos, sites = CR.fixture(name)
            ref = CR.answer(name)
            got = ctxs[name].coordination_environments(pos, sites, CR.TAU)
            info = got["info"]
            assert info["size_computed"] == 1
            assert np.all(got["status"] == CR.OK) and np.all(got["flags"] == 0)
            assert got["n"].tolist() == [r["n"] for r in ref]
            assert [v.tolist() for v in got["vertices"]] == [r["vertices"] for r in ref]
            assert [T.symbol_of(got, k) for k in range(len(sites))] == [r["symbol"] for r in ref]
            assert info["rounds"] == max(r["rounds"] for r in ref) and info["max_neighbours"] == max(r["nbr_count"] for r in ref)
            assert info["max_n"] == max(r["n"] for r in ref)
            assert CR.TOL <= 1e-9 and T.deviation(got, ref) <= CR.TOL
            if name == "sc_void":
                assert info["rounds"] == 2
            out.update({"%s/%s" % (name, k): got[k] for k in ("status", "flags", "n", "shape", "csm_best", "csm_all", "confidence")})
            for k in ("vertices", "norm_distance", "norm_angle"):
                out["%s/%s" % (name, k)] = np.concatenate([np.atleast_1d(v) for v in got[k]])
        return out
    return _two_rounds_on_contexts({n: CR.fixture(n)[0] for n in names}, round_,
                                   lambda ctx, n: ctx.coordination_environments(CR.fixture(n)[1], CR.fixture(n)[2], CR.TAU, angle_cutoff=0.31))


def probe_soap(mp):
    """Vectors of ``s65_n65`` (65 neighbours: past a wave, atoms outside the cell) and ``small_s3`` (lists beyond the staging capacity);
    site averages on the reference's golden, whole and in chunks."""
    from sitator_amd import _lib
    from tests import soap_ref as SR
    from tests import test_gpu_soap as T
    gname = str(T.GOLDEN["cases"][0])
    labels, K, W = T.GOLDEN[gname + "/labels"], int(T.GOLDEN[gname + "/n_sites"]), T.GOLDEN[gname + "/W"]
    F, M = labels.shape
    real, mobile, numbers = T.averages_input(M)
    static_idx, mobile_idx = np.where(~mobile)[0], np.where(mobile)[0]
    species = np.where(numbers[static_idx] == 8, 0, 1)
    soap_avg = T.soap_dict(2, SR.params(l_max=3, n_max=3, crossover=True))
    kw = dict(stepsize=int(T.GOLDEN[gname + "/stepsize"]), averaging=int(T.GOLDEN[gname + "/averaging"]) or None,
              avg_descriptors_per_site=int(T.GOLDEN[gname + "/avg_descriptors_per_site"]) or None)
    first, second = {}, {}
    for name in ("s65_n65", "small_s3"):
        c = T.raw_case(name)
        soap = T.soap_dict(c["Z"], c["par"])
        assert c["terms"].max() * c["par"]["n_max"] <= 1000          # the term count the bound was derived for

        def calls(ctx):
            got, cnt = ctx.soap_vectors(c["static"], c["species"], c["centers"], soap, nbr_count=True)
            assert np.array_equal(cnt, c["terms"]) and np.all(np.abs(got - c["exp"]) <= T.TOL * c["B"])
            return {name + "/vectors": got, name + "/neighbours": cnt}
        a, b = twice(lambda: plain_context(c["cell"]), calls)
        first.update(a)
        second.update(b)

    def averages(ctx):
        ctx.set_assignments(labels)
        descs, counts, nr, info = ctx.soap_site_averages(K, static_idx, species, mobile_idx, soap_avg, positions=real, **kw)
        chunked, _, _, info2 = ctx.soap_site_averages(K, static_idx, species, mobile_idx, soap_avg, positions=real,
                                                      workspace_bytes=2 * (real[0].nbytes + min(M, K) * soap_avg["n_dim"] * 8), **kw)
        V = np.concatenate([ctx.soap_vectors(real[f, static_idx], species, real[f, mobile_idx], soap_avg)[0] for f in range(F)])
        assert np.array_equal(np.repeat(np.arange(K), nr), T.GOLDEN[gname + "/desc_to_site"])
        assert descs.shape == (len(W), soap_avg["n_dim"]) and info["contributors"] == np.count_nonzero(W)
        assert np.max(np.abs(descs - W @ V)) <= T.TOL * np.max(np.abs(V))
        assert descs.tobytes() == chunked.tobytes() and info2["chunks"] > info["chunks"]
        return {"averages": descs, "averages/counts": np.asarray(counts), "averages/per_site": np.asarray(nr)}
    a, b = twice(lambda: _lib.HipContext(T.AVG_CELL), averages)
    first.update(a)
    second.update(b)
    return first, second


def probe_pca(mp):
    """Covariance of one chunk of rows + 1 by 65 columns, projection of the same shape on five components."""
    from tests import test_gpu_pca as T
    N, D = T.shape_of("chunk+1", 65)
    assert N <= 4096
    X = T.rows(N, D, 7 * N + D)
    exp_mean, B_mean = np.sum(X, axis=0) / N, np.sum(np.abs(X), axis=0) / N
    Xc = X - exp_mean
    exp_cov, B_cov = Xc.T @ Xc / (N - 1), np.abs(Xc).T @ np.abs(Xc) / (N - 1)
    X2 = T.rows(N, D, 3 * N + D)
    mean2 = X2.mean(axis=0)
    comps = np.ascontiguousarray(np.linalg.qr(np.random.default_rng(5).normal(size=(D, D)))[0][:5])
    exp_Y, B_Y = (X2 - mean2) @ comps.T, np.abs(X2 - mean2) @ np.abs(comps.T)

    def calls(ctx):
        mean, cov = ctx.pca_covariance(X)
        assert np.all(np.abs(mean - exp_mean) <= T.TOL * B_mean) and np.all(np.abs(cov - exp_cov) <= T.TOL * B_cov)
        assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes()     # symmetric bit for bit
        Y = ctx.pca_project(X2, mean2, comps)
        assert Y.shape == (N, 5) and np.all(np.abs(Y - exp_Y) <= T.TOL * B_Y)
        return dict(mean=mean, cov=cov, Y=Y)
    return twice(lambda: plain_context(T.CELL), calls)


def probe_dpc(mp):
    """The graph of ``tile+1_outlier`` (one point past a tile) at both of its fractions, and the assignment of a forest of two tiles + 1
    with several clusters and votes."""
    from tests import dpc_ref as DR
    from tests import test_gpu_dpc as T
    c = T.case("tile+1_outlier")
    Y, dist, N = c["Y"], c["dist"], c["N"]
    assert N <= 4097
    pl = T.plan()
    Na, K = 2 * pl["tile"] + 1, 7
    rho_a, delta_a, nbr_a, _ = T.forest(Na, 5, 4)
    site = np.random.default_rng(6).integers(0, K, Na)
    thr = (Na * 0.5, 0.8)
    member, clusters = DR.assign(rho_a, delta_a, nbr_a, *thr)
    assert len(clusters) > 3

    def calls(ctx):
        out = {}
        for fraction in c["fractions"]:
            dc, rank, n = DR.kernel_size(dist, fraction)
            ks, rho, delta, nbr, info = ctx.dpc_graph(Y, fraction)
            assert info["pairs"] == n == N * (N - 1) // 2
            assert np.float64(ks).view(np.uint64) == np.float64(dc).view(np.uint64)
            assert np.max((dist / dc) ** 2) <= 700.0
            exp_rho = DR.density(dist, dc)
            assert np.all(np.abs(rho - exp_rho) <= 1e-12 * exp_rho)
            exp_delta, exp_nbr = DR.delta_neighbour(dist, rho)
            assert np.array_equal(nbr, exp_nbr) and np.array_equal(delta.view(np.uint64), exp_delta.view(np.uint64))
            out.update({"%g/ks" % fraction: np.float64(ks), "%g/rho" % fraction: rho, "%g/delta" % fraction: delta, "%g/nbr" % fraction: nbr})
        got_member, got_clusters, votes = ctx.dpc_assign(rho_a, delta_a, nbr_a, thr[0], thr[1], site, K)
        assert np.array_equal(got_member, member) and np.array_equal(got_clusters, clusters)
        assert votes.shape == (K, len(clusters)) and np.array_equal(votes, DR.votes(member, site, K, len(clusters)))
        out.update(member=got_member, clusters=got_clusters, votes=votes)
        return out
    return twice(lambda: plain_context(T.CELL), calls)


def probe_pbc(mp):
    """Wrap, distances and both averages of the three cells of the reference's golden, each on one context."""
    from sitator_amd import PBCCalculator
    from tests import golden_util as G
    z = G.load("pbc_known_answers")
    first, second = {}, {}
    for name in ("ortho", "hex", "tri"):
        def calls(ctx):
            pb = PBCCalculator(z[name + "/cell"], _ctx=ctx)
            assert np.array_equal(pb.cell_centroid, z[name + "/centroid"])
            pts = z[name + "/pts"].copy()
            pb.wrap_points(pts)
            np.testing.assert_allclose(pts, z[name + "/wrapped"], rtol=1e-12, atol=1e-12)
            d = pb.distances(z[name + "/pt1"], z[name + "/pts2"])
            np.testing.assert_allclose(d, z[name + "/dists"], rtol=1e-12)
            avg, avg_w = pb.average(z[name + "/cloud"]), pb.average(z[name + "/cloud"], z[name + "/weights"])
            np.testing.assert_allclose(avg, z[name + "/avg"], rtol=0, atol=1e-10)
            np.testing.assert_allclose(avg_w, z[name + "/avg_weighted"], rtol=0, atol=1e-10)
            return {name + "/wrapped": pts, name + "/distances": d, name + "/average": avg, name + "/average_weighted": avg_w}
        a, b = twice(lambda: plain_context(z[name + "/cell"]), calls)
        first.update(a)
        second.update(b)
    return first, second


@pytest.mark.parametrize("fill", FILLS)
def test_barrier_energies(fill, monkeypatch):
    run_dirty(probe_barrier, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_pathways_and_min_image(fill, monkeypatch):
    run_dirty(probe_pathways, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_voronoi_nodes(fill, monkeypatch):
    run_dirty(probe_voronoi, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_coordination_environments(fill, monkeypatch):
    run_dirty(probe_coordenv, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_soap(fill, monkeypatch):
    run_dirty(probe_soap, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_pca(fill, monkeypatch):
    run_dirty(probe_pca, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_dpc(fill, monkeypatch):
    run_dirty(probe_dpc, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_pbc_surface(fill, monkeypatch):
    run_dirty(probe_pbc, fill, monkeypatch)


# ---- 6. frame shards and the communicator ----------------------------------------------------------------------------------------

def probe_shards(mp):
    """``LandmarkAnalysis(devices=[0, 0])`` with the mcl plugin (the exact accumulators as limbs, joined over the ranks) on the
    reference's golden, and the first operator chain of tests/shard_ref.py on the two-rank cut of its designed labels."""
    from oracle import oracle
    from sitator_amd import LandmarkAnalysis
    from tests import shard_ref as S
    from tests import test_gpu_parity as T
    oracle.lib()
    lab, K, cuts = S.designed()
    cut = cuts[sorted(cuts)[0]]
    c = T.case("c1b_tri_bcctet")
    exp = c.out("mcl")

    def round_():
        la = LandmarkAnalysis(verbose=False, devices=[0, 0], **c.kwargs("mcl"))
        st = la.run(T.make_sn(c), np.ascontiguousarray(c.frames))
        assert np.array_equal(st.traj, exp["labels"])
        m = exp["labels"] >= 0
        np.testing.assert_allclose(st.confidences[m], exp["confs"][m], rtol=1e-6)
        np.testing.assert_allclose(np.asarray(st.site_network.centers), exp["site_centers"], rtol=1e-6, atol=1e-8)
        assert int(la.n_multiple_assignments) == int(exp["n_multiple_assignments"])
        jumps = np.array(list(st.jumps()), dtype=np.int64).reshape(-1, 4)
        assert np.array_equal(jumps, exp["jumps"])
        lv = np.asarray(la.landmark_vectors)
        assert lv.shape == exp["lvecs"].shape and np.array_equal(lv != 0, exp["lvecs"] != 0)
        out = dict(labels=st.traj, confs=st.confidences, centers=np.asarray(st.site_network.centers), jumps=jumps, lvecs=lv)
        S.check_chain(oracle, S.chain_1, lab, K, cut)
        n = len(cut) - 1
        single, joined, failures = S.run_ranks(lambda t: S.chain_1(t, n if t._comm is not None else None), lab, K, cut)
        assert not failures, failures
        for i, step in enumerate(single):
            out["chain/%s/single" % step["name"]] = step["traj"]
            out["chain/%s/joined" % step["name"]] = np.concatenate([p[i]["traj"] for p in joined])
        return out
    return round_(), round_()


def probe_comm(mp):
    """Every collective of a world of one, twice on one communicator, and the mcl statistics reduced on the device through it."""
    from sitator_amd import _lib, sharding, synth
    from tests.test_gpu_kernels import _setup
    host = synth.config_host("C5")
    a = np.arange(7, dtype=np.float64) * 0.5
    b = np.array([3, -2, 9], dtype=np.int64)
    u = np.array([2 ** 63 + 5, 7], dtype=np.uint64)
    g_in = np.arange(6, dtype=np.int64).reshape(2, 3)
    x = np.linspace(0, 1, 11).reshape(11, 1)
    K = 7
    comm = sharding.RcclComm(0, 0, 1, _lib.comm_unique_id())
    ctx, frames, sm, mm, ref = _setup(host, 160, 60, seed=21)
    try:
        assert ctx.fill(check_for_zeros=False)[0] == 0
        cen = np.random.default_rng(1).uniform(0, 1, size=(K, ctx.rows_dense().shape[1]))
        ctx.set_centers(cen / np.linalg.norm(cen, axis=1)[:, None], True)
        ctx.predict(0.0, fetch=False)
        G0, seen0 = ctx.gram()
        hi0, lo0, _ = ctx.gram_limbs()
        s0, w0 = ctx.weighted_row_sums(K, weighted=True)

        def round_():
            out = dict(sum_f=comm.allreduce_sum(a), sum_i=comm.allreduce_sum(b), max_f=comm.allreduce_max(np.array([1.5])),
                       min_u=comm.ctx.comm_allreduce(u.copy(), "min"), gather=comm.allgather(g_in), bcast=comm.bcast(x, root=0))
            assert np.array_equal(out["sum_f"], a) and np.array_equal(out["sum_i"], b) and np.array_equal(out["max_f"], [1.5])
            assert np.array_equal(out["min_u"], u) and out["gather"].shape == (1, 2, 3) and np.array_equal(out["gather"][0], g_in)
            assert np.array_equal(out["bcast"], x) and comm.bcast(np.zeros((0, 4)), root=0).shape == (0, 4)
            comm.barrier()
            info = comm.info()
            assert (info["ranks"], info["rank"], info["device"]) == (1, 0, 0) and info["rccl_version"] > 0
            ctx.comm_attach(comm.ctx)
            try:
                G1, seen1 = ctx.gram()
                hi1, lo1, _ = ctx.gram_limbs()
                s1, w1 = ctx.weighted_row_sums(K, weighted=True)
            finally:
                ctx.comm_attach(None)
            assert np.array_equal(G0, G1) and np.array_equal(seen0, seen1) and np.array_equal(hi0, hi1) and np.array_equal(lo0, lo1)
            assert np.array_equal(s0, s1) and np.array_equal(w0, w1) and np.array_equal(G0, G0.T) and np.count_nonzero(G0) > 0
            out.update(gram=G1, seen=seen1, hi=hi1, lo=lo1, sums=s1, wsum=w1)
            return out
        return round_(), round_()
    finally:
        ctx.close()
        comm.close()


@pytest.mark.parametrize("fill", FILLS)
def test_frame_shards(fill, monkeypatch):
    run_dirty(probe_shards, fill, monkeypatch)


@pytest.mark.parametrize("fill", FILLS)
def test_comm_world_of_one(fill, monkeypatch):
    run_dirty(probe_comm, fill, monkeypatch)


# ---- 7. nothing is left out ------------------------------------------------------------------------------------------------------

def test_every_entry_point_that_allocates_has_a_probe():
    """The list in this module's docstring against the ``sit_*`` symbols of include/*.h: every exported entry point is either reached
    by a probe or named in ``EXEMPT`` (it neither allocates nor carves), nothing is named that the headers do not export, and every
    probe named there has its test in this module."""
    exported = set()
    for header in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
        exported |= set(re.findall(r"\b(sit_[a-z0-9_]+)\s*\(", text))
    assert len(exported) >= 100
    listing = __doc__[__doc__.index("PROBES = {"):]
    probed = set(re.findall(r"\bsit_[a-z0-9_]+", listing))
    names = re.findall(r'^ "(\w+)":', listing, flags=re.M)
    assert len(names) >= 25
    for name in names:
        assert "probe_" + name in globals(), name
    assert not (probed & set(EXEMPT)), sorted(probed & set(EXEMPT))
    assert not (probed | set(EXEMPT)) - exported, sorted((probed | set(EXEMPT)) - exported)
    missing = exported - probed - set(EXEMPT)
    assert not missing, "entry points without a probe: %s" % sorted(missing)
