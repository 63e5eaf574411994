"""GPU: ``sit_density`` (density.hip: the counts through the LDS table of a workgroup and its spill path, the direct form, the
smoothing over a haloed tile in LDS and from memory, the peaks and their compaction) and ``IonicDensity`` on top of it, against
the numpy restatement of tests/density_ref.py (itself pinned to designed inputs by tests/test_density_ref.py and to density_plan.h
by tests/test_density_plan.py).

Counts are integers and the smoothing is a gather whose every product and sum is the same float64 operation in the same order on
both sides: everything is compared on its bytes, there is no tolerance."""
import numpy as np
import pytest

from tests import density_ref as R
from tests import golden_util as G
from tests import msd_ref as M
from tests.test_gpu_msd import Context, DRIFT, wrapped_walk
from tests.test_gpu_vibfreq import resident_frames

pytestmark = pytest.mark.gpu


def device(ctx, x, atoms, grid, **kw):
    from sitator_amd import _lib_density
    return _lib_density.density(ctx, atoms, grid, positions=x, **kw)


def same_bytes(got, exp):
    return got is not None and got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()


def walk(F, A, seed, cell):
    return wrapped_walk(F, A, seed, cell, drift=DRIFT)[0]


# (cell, grid, frames, atoms of the selection, frame_stride): the grids, the frame counts around a run of 64, the selections below and
# beyond a workgroup's threads, the strides of the issue, each at least once and mixed
CASES = {
    "one_voxel_one_frame_one_atom": ("ortho", (1, 1, 1), 1, 1, 1),
    "two_frames_64_atoms": ("hex", (2, 3, 5), 2, 64, 1),
    "one_short_of_a_run_130_atoms": ("triclinic", (17, 16, 33), 63, 130, 1),
    "a_run_one_atom_stride_3": ("ortho", (17, 16, 33), 64, 1, 3),
    "past_a_run_by_one": ("hex", (64, 48, 40), 65, 64, 1),
    "seven_runs_130_atoms_stride_3": ("triclinic", (64, 48, 40), 389, 130, 3),
    "seven_runs_64_atoms": ("ortho", (2, 3, 5), 389, 64, 1),
    "stride_beyond_the_frames": ("hex", (17, 16, 33), 389, 64, 1000),
    "seven_runs_one_atom": ("triclinic", (1, 1, 1), 389, 1, 1),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_are_the_restatement(name):
    cell_name, grid, F, n_sel, stride = CASES[name]
    cell = M.CELLS[cell_name]
    x = walk(F, n_sel + 3, 300 + F + n_sel, cell)
    atoms = 1 + np.arange(n_sel)[::-1]                              # a list, not a range: the order of a selection does not matter
    exp, taken, skipped = R.counts(x, cell, atoms, grid, stride)
    assert taken == (F - 1) // stride + 1 and skipped == 0 and exp.sum() == taken * n_sel
    with Context(cell) as ctx:
        got = {form: device(ctx, x, atoms, grid, frame_stride=stride, form=form) for form in (0, 1, 2)}
        again = device(ctx, x, atoms, grid, frame_stride=stride)
    for g in list(got.values()) + [again]:
        assert same_bytes(g[0], exp) and g[1] is None and g[2:] == (taken, 0)


def test_every_atom_in_one_voxel_for_every_frame():
    """The most contention there is: one key in every table, one address in memory."""
    cell, grid = M.TRICLINIC, (17, 16, 33)
    F, n = 200, 64
    x = np.ascontiguousarray(np.broadcast_to(np.array([0.3, 0.45, 0.7]) @ cell, (F, n, 3)))
    v = int(R.voxel(x[0, 0], R.cell_inverse(cell), grid))
    with Context(cell) as ctx:
        for form in (1, 2):
            c, _, taken, skipped = device(ctx, x, np.arange(n), grid, form=form)
            assert (taken, skipped) == (F, 0) and c.reshape(-1)[v] == F * n and c.sum() == F * n


def test_more_voxels_in_a_run_than_the_table_has_slots():
    """Atoms spread over the cell, a new place in every frame: a run of 64 frames x 130 atoms meets more distinct voxels than the
    table has slots, so entries go to memory on their own."""
    cell, grid = M.HEX, (64, 48, 40)
    F, n = 65, 130
    x = np.random.default_rng(8).uniform(0.0, 1.0, size=(F, n, 3)) @ cell
    exp, taken, _ = R.counts(x, cell, np.arange(n), grid)
    first_run = R.voxel(x[:R.RUN], R.cell_inverse(cell), grid)
    assert len(np.unique(first_run)) > R.SLOTS + 2000                # beyond the slots by far more than the probe limit could hide
    with Context(cell) as ctx:
        got = [device(ctx, x, np.arange(n), grid, form=form) for form in (0, 1, 2, 2)]
    assert all(same_bytes(g[0], exp) and g[2] == taken for g in got)


def test_atoms_a_thousand_cells_outside_the_box():
    cell = np.diag([8.0, 4.0, 16.0])
    rng = np.random.default_rng(6)
    F, n = 70, 5
    x = rng.integers(0, 1 << 22, size=(F, n, 3)) / float(1 << 20) % np.diag(cell)
    moved = np.ascontiguousarray(x + rng.integers(-1000, 1001, size=(F, n, 3)) * np.diag(cell)[None, None, :])
    grid = (16, 8, 32)
    exp = R.counts(x, cell, np.arange(n), grid)[0]
    assert exp.sum() == F * n
    with Context(cell) as ctx:
        assert same_bytes(device(ctx, moved, np.arange(n), grid)[0], exp) and same_bytes(device(ctx, x, np.arange(n), grid)[0], exp)


def test_nan_and_inf_are_skipped_and_counted():
    cell, grid = M.ORTHO, (5, 4, 6)
    x = np.array(walk(130, 6, 9, cell))
    x[5, 1, 2] = np.nan
    x[7, 4, 0] = np.inf
    x[7, 4, 1] = -np.inf
    x[129, 0, 1] = np.nan
    x[64, 3] = np.nan                                             # unselected: not looked at
    atoms = np.array([0, 1, 2, 4, 5])
    exp, taken, skipped = R.counts(x, cell, atoms, grid)
    assert skipped == 3 and exp.sum() == 130 * 5 - 3
    with Context(cell) as ctx:
        for form in (1, 2):
            got = device(ctx, x, atoms, grid, form=form)
            assert same_bytes(got[0], exp) and got[2:] == (130, 3)
        every = device(ctx, x, np.arange(6), grid)
    assert every[3] == 4 and every[0].sum() == 130 * 6 - 4


def test_points_on_voxel_boundaries_and_just_below_the_upper_face():
    """A cell with power-of-two edges: s = x / edge exactly.  Points on every voxel boundary go to the upper voxel; s = -1e-17
    and s = 1 - 2^-53 go to the last voxel of every axis."""
    edges = np.array([8.0, 4.0, 16.0])
    cell = np.diag(edges)
    for grid in ((8, 4, 16), (1, 3, 7), (1024, 1, 2)):
        n = np.array(grid)
        k = np.stack(np.meshgrid(*[np.arange(min(g, 16)) for g in grid], indexing="ij"), axis=-1).reshape(-1, 3)
        s = np.concatenate([k / n.astype(np.float64), [[-1e-17] * 3, [1.0 - 2.0 ** -53] * 3, [-1e-17, 0.0, 1.0 - 2.0 ** -53]]])
        x = np.ascontiguousarray((s * edges)[None])                   # one frame, a point per atom
        v = R.voxel(x[0], R.cell_inverse(cell), grid)
        V = int(n.prod())
        assert v[-3] == V - 1 and v[-2] == V - 1 and v[-1] == ((n[0] - 1) * n[1] + 0) * n[2] + n[2] - 1
        if grid == (8, 4, 16):
            assert np.array_equal(v[:len(k)], (k[:, 0] * 4 + k[:, 1]) * 16 + k[:, 2])
        exp = R.counts(x, cell, np.arange(len(s)), grid)[0]
        with Context(cell) as ctx:
            for form in (1, 2):
                assert same_bytes(device(ctx, x, np.arange(len(s)), grid, form=form)[0], exp)


@pytest.mark.parametrize("stride", [1, 3])
def test_the_smallest_workspace_cap(stride):
    """A host array goes up in windows of whole runs: with the smallest cap the plan accepts - one run - the same bytes as with
    everything at once; one byte below it is refused."""
    from sitator_amd import _lib_density
    cell, grid = M.HEX, (17, 16, 33)
    F, A = 389, 12
    x = walk(F, A, 21, cell)
    atoms = np.array([0, 3, 4, 11])
    exp, taken, _ = R.counts(x, cell, atoms, grid, stride)
    one = -(-(((R.RUN - 1) * stride + 1) * A * 24) // 256) * 256
    least = R.plan(F, A, len(atoms), grid, stride, cap=one)
    assert least["window"] == R.RUN and least["n_windows"] == -(-taken // R.RUN) >= 3 and R.plan(F, A, len(atoms), grid, stride, cap=one - 1) is None
    assert _lib_density.density_plan(F, A, len(atoms), grid, stride, workspace_bytes=one)["n_windows"] == least["n_windows"]
    with Context(cell) as ctx:
        whole = device(ctx, x, atoms, grid, frame_stride=stride)
        capped = device(ctx, x, atoms, grid, frame_stride=stride, workspace_bytes=one)
        two = device(ctx, x, atoms, grid, frame_stride=stride, workspace_bytes=2 * one + 300)
        with pytest.raises(ValueError, match="one run"):
            device(ctx, x, atoms, grid, frame_stride=stride, workspace_bytes=one - 1)
    for got in (whole, capped, two):
        assert same_bytes(got[0], exp) and got[2] == taken


@pytest.fixture(scope="module")
def crowd():
    """150 frames of 30 atoms wrapped into the cell resident frames come with, and their counts on a 17 x 16 x 33 grid, once."""
    cell = Context.resident_cell()
    x = walk(150, 30, 35, cell)
    atoms = np.array([3, 17, 20, 21, 29, 0, 1])
    grid = (17, 16, 33)
    exp = R.counts(x, cell, atoms, grid)[0]
    for arr in (x, exp):
        arr.flags.writeable = False
    return dict(cell=cell, x=x, atoms=atoms, grid=grid, counts=exp)


def test_smoothing_is_the_restatement(crowd):
    from sitator_amd import gaussian_stencil
    c = crowd
    rng = np.random.default_rng(4)
    box = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    stencils = {
        "one_tap": (np.zeros((1, 3), dtype=np.int64), np.array([1.0])),
        "one_tap_elsewhere": (np.array([[-8, 7, 16]]), np.array([-0.75])),
        "27_taps": (box, rng.normal(size=27)),                        # signed weights: the order of the sum shows
        "beyond_the_lds_tile": (np.array([[8, 7, 0], [-8, -7, 3], [0, 1, 0], [0, 0, -16]]), np.array([0.5, 0.25, -2.0, 1e-3])),
    }
    # a Gaussian of a few hundred taps on a grid smaller than the tile with its halo: the staged neighbourhood wraps round the grid
    small = (9, 9, 11)
    gauss = gaussian_stencil(c["cell"], small, 1.5, 3.0)
    halo = R.halo(gauss[0], small)
    small_plan = R.plan(150, 30, 7, small, n_taps=len(gauss[0]), halo3=halo)
    assert 200 <= len(gauss[0]) <= 1000 and all(small_plan["ext"][a] > small[a] for a in range(3)) and small_plan["smooth_lds"] > 0
    small_counts = R.counts(c["x"], c["cell"], c["atoms"], small)[0]
    assert R.plan(150, 30, 7, c["grid"], n_taps=4, halo3=(8, 7, 16))["smooth_lds"] == 0      # and this one reads memory
    with Context(c["cell"]) as ctx:
        for name, (taps, w) in stencils.items():
            exp = R.smooth(c["counts"], taps, w)
            for form in (1, 2):
                got = device(ctx, c["x"], c["atoms"], c["grid"], taps=taps, weights=w, form=form)
                assert same_bytes(got[0], c["counts"]) and same_bytes(got[1], exp), name
            if name == "one_tap":
                assert same_bytes(got[1], c["counts"].astype(np.float64))
            if name == "27_taps":
                assert not np.signbit(got[1][got[1] == 0.0]).any() and (got[1] == 0.0).sum() > got[1].size // 2    # +0 where nothing is near
        taps, w = gauss
        got = device(ctx, c["x"], c["atoms"], small, taps=taps, weights=w)
        assert same_bytes(got[0], small_counts) and same_bytes(got[1], R.smooth(small_counts, taps, w))
        total = float(small_counts.sum())
        assert abs(float(got[1].astype(np.longdouble).sum()) - total * float(w.astype(np.longdouble).sum())) <= len(w) * R.U * total
        # a second plane that stays empty, and a grid of one voxel
        short = device(ctx, c["x"], c["atoms"], (1, 1, 1), taps=[[0, 0, 0], [0, 0, 0]], weights=[0.5, 0.25])
        assert short[1].tolist() == [[[[0.75 * 150 * 7]]]]


def test_limits_are_errors_not_faults(crowd):
    from sitator_amd import _lib_density
    c = crowd
    ok = dict(atoms=c["atoms"], grid=c["grid"])

    def call(ctx, x, **kw):
        args = dict(ok, **kw)
        return device(ctx, x, args.pop("atoms"), args.pop("grid"), **args)

    with Context(frames=np.array(c["x"])) as ctx:
        version = ctx.labels_version
        assert same_bytes(call(ctx, None)[0], c["counts"])           # the resident frames
        for bad in (dict(grid=(0, 4, 4)), dict(grid=(4, 1025, 4)), dict(grid=(4, 4, -1)), dict(grid=(1024, 1024, 129)), dict(frame_stride=0),
                    dict(frame_stride=-2), dict(atoms=[]), dict(atoms=[0, 30]), dict(atoms=[-1]), dict(atoms=[3, 1 << 40]),
                    dict(atoms=np.zeros((1 << 20) + 1, dtype=np.int64)), dict(form=3), dict(form=-1), dict(workspace_bytes=-1),
                    dict(n_classes=2), dict(n_classes=0), dict(n_classes=17),
                    dict(taps=[[9, 0, 0]], weights=[1.0]), dict(taps=[[0, -8, 0]], weights=[1.0]), dict(taps=[[0, 0, 17]], weights=[1.0]),
                    dict(taps=[[0, 0, 1 << 40]], weights=[1.0]), dict(taps=[[0, 0, 0]], weights=[np.inf]), dict(taps=[[0, 0, 0]], weights=[np.nan]),
                    dict(taps=np.zeros(((1 << 15) + 1, 3), dtype=np.int64), weights=np.zeros((1 << 15) + 1)),
                    dict(site_class=[0, 0, 0], n_classes=2)):       # no valid labels on this context
            with pytest.raises(ValueError):
                call(ctx, None, **bad)
        with pytest.raises(ValueError):                              # a cap below one run of a host array
            call(ctx, np.array(c["x"]), workspace_bytes=100)
        assert same_bytes(call(ctx, None, workspace_bytes=100)[0], c["counts"])    # the resident frames need no window
        with pytest.raises(ValueError):                              # F other than the resident frames'
            ctx.F += 1
            try:
                call(ctx, None)
            finally:
                ctx.F -= 1
        with pytest.raises(ValueError, match="resident"):            # A other than the resident frames'
            ctx.A += 1
            try:
                call(ctx, None)
            finally:
                ctx.A -= 1
        with pytest.raises(ValueError):                              # no frame at all
            _lib_density.density(ctx, [0], (2, 2, 2), positions=np.zeros((0, 2, 3)))
        assert same_bytes(call(ctx, None, frame_stride=1 << 40)[0], R.counts(c["x"], c["cell"], c["atoms"], c["grid"], 1 << 40)[0])
        assert same_bytes(call(ctx, None)[0], c["counts"]) and ctx.labels_version == version        # and the context still works
        assert np.array_equal(resident_frames(ctx), c["x"])
    with Context(c["cell"]) as ctx:
        with pytest.raises(ValueError):                              # nothing resident
            call(ctx, None)
    from sitator_amd import IonicDensity
    flat = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [5.0, 7.0, 9.0]])
    for cell in (flat, np.zeros((3, 3))):
        with pytest.raises(ValueError):                              # numpy's inverse refuses it, or sit_density does
            IonicDensity(grid=(4, 4, 4)).compute(np.array(c["x"]), cell, [0, 1])


def test_peaks_are_the_restatement():
    from sitator_amd import _lib_density
    rng = np.random.default_rng(9)
    grids = []
    for shape in ((1, 1, 1), (1, 1, 2), (2, 2, 2), (1, 4, 2), (3, 3, 3), (5, 4, 6), (2, 1, 7), (17, 16, 5)):
        grids.append(rng.integers(0, 4, size=shape).astype(float))   # many ties
        grids.append(rng.normal(size=shape))
        grids.append(np.zeros(shape))
        withnan = rng.integers(0, 3, size=shape).astype(float)
        withnan.reshape(-1)[rng.integers(0, withnan.size)] = np.nan
        grids.append(withnan)
    with Context(M.ORTHO) as ctx:
        for g in grids:
            for thr in (0.0, 0.5, -np.inf):
                got = _lib_density.density_peaks(ctx, g, thr)
                assert got.dtype == np.int64 and np.array_equal(got, R.peaks(g, thr)), (g.shape, thr)
        assert list(_lib_density.density_peaks(ctx, np.zeros((4, 5, 3)), 0.0)) == [0]
        assert len(_lib_density.density_peaks(ctx, np.full((4, 5, 3), np.nan), 0.0)) == 0
        # more peaks than the first request has room for, over many workgroups: every voxel with three even coordinates
        big = np.zeros((128, 128, 64))
        big[::2, ::2, ::2] = 1.0
        got = _lib_density.density_peaks(ctx, big, 0.5)
        assert len(got) == 64 * 64 * 32 > 1 << 16 and np.array_equal(got, np.flatnonzero(big.reshape(-1)))
        with pytest.raises(ValueError):
            _lib_density.density_peaks(ctx, np.zeros((1025, 1, 1)), 0.0)


def analysis():
    from sitator_amd import LandmarkAnalysis, SiteNetwork, Structure, synth
    host = synth.config_host("C1")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 300, seed=17, p_hop=1.0 / 40)
    sn = SiteNetwork(Structure(ref, host.cell), sm, mm)
    sn.centers = host.centers
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False)
    st = la.run(sn, frames)
    return la, st, np.ascontiguousarray(frames), np.asarray(host.cell, dtype=np.float64), sm, mm


def test_operator_on_the_frames_and_labels_an_analysis_left_resident(tmp_path):
    from sitator_amd import DensityResult, IonicDensity, gaussian_stencil
    la, st, frames, cell, sm, mm = analysis()
    ctx = la._ctx
    mobile = np.where(mm)[0]
    labels = st._traj.copy()
    n_sites = st.site_network.n_sites
    assert (labels < 0).any() and (labels >= 0).any() and n_sites >= 3
    version = ctx.labels_version
    op = IonicDensity(grid=(12, 11, 13), sigma=0.8, cutoff=3.0, frame_stride=2)
    taps, w = gaussian_stencil(cell, (12, 11, 13), 0.8, 3.0)
    assert len(taps) > 27
    exp, taken, _ = R.counts(frames, cell, mobile, (12, 11, 13), 2)
    got = op.compute_for_analysis(la)
    assert isinstance(got, DensityResult) and got.class_names == ("all",) and got.grid == (12, 11, 13)
    for r in (got, op.compute(frames, cell, mm), op.compute_for_analysis(la, mask=mm), op.compute_for_analysis(la, mask=mobile)):
        assert same_bytes(r.counts, exp) and same_bytes(r.smoothed, R.smooth(exp, taps, w)) and (r.n_frames, r.skipped) == (taken, 0)
    assert got.voxel_volume == abs(np.linalg.det(cell)) / (12 * 11 * 13) and np.array_equal(got.density, exp / (float(taken) * got.voxel_volume))
    static = IonicDensity(spacing=0.9).compute_for_analysis(la, mask=sm)
    n = tuple(int(v) for v in np.clip(np.ceil(np.linalg.norm(cell, axis=1) / 0.9), 1, 1024))
    assert static.grid == n and static.smoothed is None and same_bytes(static.counts, R.counts(frames, cell, np.where(sm)[0], n)[0])
    # the planes of the labels
    two = op.compute_for_trajectory(la)
    lab = R.counts(frames, cell, mobile, (12, 11, 13), 2, labels, np.zeros(n_sites, dtype=np.int32), 2)[0]
    assert two.class_names == ("assigned", "unassigned") and same_bytes(two.counts, lab)
    assert np.array_equal(two.counts.sum(axis=0, keepdims=True), exp) and two.counts[1].sum() == (labels[::2] < 0).sum()
    every = IonicDensity(grid=(12, 11, 13)).compute_for_trajectory(la, st)
    assert every.counts[1].sum() == (st._traj < 0).sum() and every.counts[0].sum() == (st._traj >= 0).sum()
    classes = np.arange(n_sites) % 3
    three = op.compute_for_trajectory(la, st, classes=classes)
    assert three.class_names == ("class 0", "class 1", "class 2", "unassigned")
    assert same_bytes(three.counts, R.counts(frames, cell, mobile, (12, 11, 13), 2, labels, classes, 4)[0])
    assert same_bytes(three.smoothed, R.smooth(three.counts, taps, w))
    st.site_network.site_types = 5 - 2 * (np.arange(n_sites) % 2)            # types 5, 3: ascending order is 3, 5
    typed = op.compute_for_trajectory(la, classes="site_types")
    assert typed.class_names == ("type 3", "type 5", "unassigned")
    assert same_bytes(typed.counts, R.counts(frames, cell, mobile, (12, 11, 13), 2, labels, 1 - np.arange(n_sites) % 2, 3)[0])
    # sit_density's own range check of site_class (the operator's classes never reach it), on valid labels
    from sitator_amd import _lib_density
    ok_class = np.zeros(n_sites, dtype=np.int32)
    assert same_bytes(_lib_density.density(ctx, mobile, (12, 11, 13), frame_stride=2, site_class=ok_class, n_classes=2)[0], lab)
    for k, value, n_classes in ((0, 1, 2), (n_sites - 1, 1, 2), (1, -1, 2), (2, 3, 4), (0, 1 << 20, 16)):
        bad_class = ok_class.copy()
        bad_class[k] = value                                       # n_classes - 1 is the unassigned plane: no site's
        with pytest.raises(ValueError, match="class"):
            _lib_density.density(ctx, mobile, (12, 11, 13), site_class=bad_class, n_classes=n_classes)
    with pytest.raises(ValueError):                                # the selection is the label columns, in order
        _lib_density.density(ctx, mobile[::-1], (12, 11, 13), site_class=ok_class, n_classes=2)
    with pytest.raises(ValueError):
        _lib_density.density(ctx, mobile[:-1], (12, 11, 13), site_class=ok_class, n_classes=2)
    for bad in ("sites", np.arange(n_sites + 1), -np.ones(n_sites, dtype=np.int64), np.arange(n_sites) * 16):
        with pytest.raises(ValueError):
            op.compute_for_trajectory(la, classes=bad)
    # nothing moved
    assert ctx.labels_version == version and np.array_equal(resident_frames(ctx), frames)
    assert np.array_equal(ctx.assignments()[0].reshape(labels.shape), labels) and np.array_equal(st._traj, labels)
    # peaks on the device, sites, the cube file
    v, fr, pos, values = two.peaks(0.05, plane=0)
    grid0 = two.smoothed[0]
    assert np.array_equal(np.sort(v), R.peaks(grid0, 0.05 * grid0.max())) and len(v) >= 1
    assert np.array_equal(values, grid0.reshape(-1)[v]) and np.all(np.diff(values) <= 0) and np.allclose(pos, fr @ cell)
    match = two.match_sites(st.site_network, plane=0)
    centers = np.asarray(st.site_network.centers)
    assert np.array_equal(match["peak_voxels"], v) and np.array_equal(match["site_density"], two.density[0].reshape(-1)[two.voxel_of(centers)])
    from sitator_amd import PBCCalculator
    dist = np.array([PBCCalculator(cell).distances(centers[s], pos) for s in range(n_sites)])
    assert np.array_equal(match["site_peak"], dist.argmin(axis=1)) and np.array_equal(match["site_peak_distance"], dist.min(axis=1))
    assert np.array_equal(match["peak_site"], dist.argmin(axis=0)) and np.array_equal(match["peak_site_distance"], dist.min(axis=0))
    two.write_cube(str(tmp_path / "rho.cube"), st.site_network.structure)
    # an edited label beyond the sites (st.traj hands out the array: the labels are uploaded again, by the trajectory, not by the density)
    st.traj[8, 1] = n_sites + 2
    with pytest.raises(IndexError, match="index %d is out of bounds" % (n_sites + 2)):
        op.compute_for_trajectory(la, st)
    st.traj[8, 1] = -2
    with pytest.raises(ValueError):
        op.compute_for_trajectory(la, st)
    st.traj[8, 1] = labels[8, 1]
    assert same_bytes(op.compute_for_trajectory(la, st).counts, lab)
    assert np.array_equal(ctx.assignments()[0].reshape(labels.shape), labels) and np.array_equal(resident_frames(ctx), frames)


def test_operator_refuses_frame_shards():
    from sitator_amd import IonicDensity, LandmarkAnalysis, SiteNetwork, Structure
    c = G.Case("c1_hex_scgrid")
    sn = SiteNetwork(Structure(c.ref_positions, c.cell), c.static_mask, c.mobile_mask)
    sn.centers = c.centers
    sn.vertices = c.vertices
    la = LandmarkAnalysis(verbose=False, devices=[0, 0], **c.kwargs("dotprod"))
    la.run(sn, np.ascontiguousarray(c.frames))
    with pytest.raises(NotImplementedError):
        IonicDensity(grid=(4, 4, 4)).compute_for_analysis(la)
    with pytest.raises(NotImplementedError):
        IonicDensity(grid=(4, 4, 4)).compute_for_trajectory(la)
