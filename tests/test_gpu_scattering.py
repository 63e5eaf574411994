"""GPU: ``sit_scattering`` (scattering.hip: the fractional coordinates, the density modes over tiles of power tables in LDS, the
coherent products under the fixed tree, the self part, the block sums) and ``IntermediateScattering`` / ``StructureFactor`` on top of
it, against the numpy restatement of tests/scattering_ref.py (itself pinned to a long-double evaluation and closed forms by
tests/test_scattering_ref.py and to scattering_plan.h by tests/test_scattering_plan.py).

The raw sums are compared on their bytes: every product and every sum is the same float64 operation in the same order on both
sides, so there is no tolerance.  Where a NaN is put in on purpose, a NaN need only be a NaN."""
import numpy as np
import pytest

from tests import golden_util as G
from tests import msd_ref as R
from tests import scattering_ref as S
from tests.test_gpu_msd import Context, DRIFT, wrapped_walk
from tests.test_gpu_vibfreq import resident_frames

pytestmark = pytest.mark.gpu

Q_EDGE = np.array([[0, 0, 0], [32, 0, 0], [-32, 0, 0], [0, 32, 0], [0, -32, 0], [0, 0, 32], [0, 0, -32], [-32, 32, -32], [1, -2, 3],
                   [-1, 0, 0], [0, -7, 2]])


def q_list(seed, n=4, most=32):
    return np.concatenate([Q_EDGE, np.random.default_rng(seed).integers(-most, most + 1, size=(n, 3))])


def device(ctx, x, a, b, same, q, lags, stride, **kw):
    from sitator_amd import _lib_scattering
    return _lib_scattering.scattering(ctx, a, b, q, lags, positions=x, same=same, origin_stride=stride, **kw)


def lags_of(F, extra=()):
    return np.unique(np.clip([0, 1, F - 1] + list(extra), 0, F - 1))


def same_bytes(got, exp):
    return got.dtype == exp.dtype == np.complex128 and got.shape == exp.shape and got.tobytes() == exp.tobytes()


def same_but_nan(got, exp):
    g, e = got.view(np.float64), exp.view(np.float64)
    nan = np.isnan(e)
    return got.shape == exp.shape and np.array_equal(np.isnan(g), nan) and g[~nan].tobytes() == e[~nan].tobytes()


# (cell, F, n_a, n_b or None for one selection, stride, further lags, q vectors beyond the designed ones, their largest index)
CASES = {
    "one_frame_one_atom": ("ortho", 1, 1, None, 1, (), 2, 32),
    "two_frames_two_lists": ("hex", 2, 3, 64, 1, (), 3, 32),
    "five_frames_past_the_atom_tile": ("triclinic", 5, 65, None, 3, (2,), 3, 32),
    "past_a_block_by_one": ("ortho", S.BLOCK + 1, 3, 130, 1, (64,), 3, 32),
    "past_a_block_130_atoms": ("hex", S.BLOCK + 1, 130, None, 1, (), 2, 32),
    "more_q_than_a_tile": ("triclinic", 40, 64, None, 3, (7,), 2 * S.QTILE + 30, 5),
    "stride_3_two_blocks": ("triclinic", 3 * S.BLOCK + 5, 2, 3, 3, (5, 100), 4, 32),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_sums_are_the_restatement(name):
    cell_name, F, n_a, n_b, stride, extra, n_random, most = CASES[name]
    cell = R.CELLS[cell_name]
    same = n_b is None
    x, _, _ = wrapped_walk(F, n_a + (n_b or 0), 200 + F + n_a, cell, drift=DRIFT)
    a = np.arange(n_a)
    b = a if same else n_a + np.arange(n_b)
    q, lags = q_list(F + n_a, n_random, most), lags_of(F, extra)
    ss, cs = S.sums(x, cell, a, b, same, q, lags, stride)
    origins = np.array([S.n_origins(F, int(t), stride) for t in lags])
    assert np.all(ss[lags == 0] == origins[0] * n_a) and np.all(np.abs(cs[:, 0] - origins * n_a * len(b)) < 1e-6 * origins * n_a * len(b))
    with Context(cell) as ctx:
        got = device(ctx, x, a, b, same, q, lags, stride)
        again = device(ctx, x, a, b, same, q, lags, stride)
        only_s = device(ctx, x, a, b, same, q, lags, stride, coherent_part=False)
        only_c = device(ctx, x, a, b, same, q, lags, stride, self_part=False)
    assert same_bytes(got[0], ss) and same_bytes(got[1], cs)
    assert same_bytes(again[0], got[0]) and same_bytes(again[1], got[1])          # two calls, the same bytes
    assert only_s[1] is None and same_bytes(only_s[0], ss) and only_c[0] is None and same_bytes(only_c[1], cs)


@pytest.fixture(scope="module")
def crowd():
    """F = 150 (two blocks of origins), 30 atoms wrapped into the cell resident frames come with; the reference of two lists of
    them over ten q vectors and five lags, computed once."""
    cell = Context.resident_cell()
    x, _, _ = wrapped_walk(150, 30, 35, cell, drift=DRIFT)
    a, b = np.array([3, 17, 20, 21, 29]), np.array([0, 1, 5, 9, 10, 11, 28])
    q = np.array([[0, 0, 0], [1, 0, 0], [0, -2, 1], [3, 3, -3], [-6, 0, 2], [0, 0, 5], [2, -1, 0], [1, 1, 1], [-4, 4, 0], [0, 6, -6]])
    lags = lags_of(150, (5, 20))
    ss, cs = S.sums(x, cell, a, b, False, q, lags, 1)
    for arr in (x, ss, cs):
        arr.flags.writeable = False
    return dict(cell=cell, x=x, a=a, b=b, q=q, lags=lags, ss=ss, cs=cs)


def test_resident_frames_are_the_host_array(crowd):
    """The lists as columns of the resident frames (the other atoms holding NaN) and of the same array on the host: bit for bit, and
    the context stays as it was."""
    c = crowd
    mask = np.zeros(30, dtype=bool)
    mask[c["a"]] = mask[c["b"]] = True
    holed = np.where(mask[None, :, None], c["x"], np.nan)
    with Context(frames=holed) as ctx:
        version = ctx.labels_version
        host = device(ctx, holed, c["a"], c["b"], False, c["q"], c["lags"], 1, coherent_part=True, self_part=True)
        res = device(ctx, None, c["a"], c["b"], False, c["q"], c["lags"], 1)
        assert ctx.labels_version == version and np.array_equal(resident_frames(ctx), holed, equal_nan=True)
    for got in (host, res):
        assert same_bytes(got[0], c["ss"]) and same_bytes(got[1], c["cs"])


@pytest.mark.parametrize("stride", [1, 3])
def test_a_small_workspace_is_the_default(crowd, stride):
    """A cap that leaves three q vectors, sixteen frames and three lags at a time, and the smallest one the call takes - one q
    vector, one frame, one lag: the same bytes as with everything held."""
    c = crowd
    F, n_q, n_lags = 150, len(c["q"]), len(c["lags"])
    H = S.h_max(c["q"])
    ss, cs = (c["ss"], c["cs"]) if stride == 1 else S.sums(c["x"], c["cell"], c["a"], c["b"], False, c["q"], c["lags"], stride)
    blocks = S.n_blocks(S.n_origins(F, 0, stride))
    one = 1024 + 2 * F * 16 + 12 * 24 + blocks * 16
    some = 1024 + 4 * (2 * F * 16 + blocks * 16)
    p = S.plan(F, 5, 7, False, n_q, H, n_lags, stride, True, True, some)
    assert p["n_q_batches"] >= 3 and -(-F // p["window"]) >= 3 and (p["lags_per_launch"] < n_lags or stride > 1)
    least = S.plan(F, 5, 7, False, n_q, H, n_lags, stride, True, True, one)
    assert (least["q_batch"], least["window"], least["lags_per_launch"]) == (1, 1, 1)
    with Context(c["cell"]) as ctx:
        whole = device(ctx, c["x"], c["a"], c["b"], False, c["q"], c["lags"], stride)
        capped = device(ctx, c["x"], c["a"], c["b"], False, c["q"], c["lags"], stride, workspace_bytes=some)
        smallest = device(ctx, c["x"], c["a"], c["b"], False, c["q"], c["lags"], stride, workspace_bytes=one)
        with pytest.raises(ValueError):
            device(ctx, c["x"], c["a"], c["b"], False, c["q"], c["lags"], stride, workspace_bytes=one - 1)
        self_only = device(ctx, c["x"], c["a"], c["b"], False, c["q"], c["lags"], stride, workspace_bytes=1024 + blocks * 16, coherent_part=False)
    assert same_bytes(whole[0], ss) and same_bytes(whole[1], cs)
    for got in (capped, smallest):
        assert same_bytes(got[0], whole[0]) and same_bytes(got[1], whole[1])
    assert same_bytes(self_only[0], ss)


def test_atoms_many_cells_outside_the_box():
    """An orthorhombic cell with power-of-two edges and positions on a grid of 2^-20: atoms moved by up to a thousand cell vectors,
    a different number in every frame, give the same bytes as the atoms in the box."""
    cell = np.diag([8.0, 4.0, 16.0])
    rng = np.random.default_rng(6)
    F, n = 20, 5
    x = rng.integers(0, 1 << 22, size=(F, n, 3)) / float(1 << 20)
    moved = np.ascontiguousarray(x + rng.integers(-1000, 1001, size=(F, n, 3)) * np.diag(cell)[None, None, :])
    q, lags = q_list(11, 6), [0, 1, 5, 19]
    a, b = np.array([0, 1, 2]), np.array([3, 4])
    ss, cs = S.sums(x, cell, a, b, False, q, lags, 1)
    with Context(cell) as ctx:
        got = device(ctx, moved, a, b, False, q, lags, 1)
        inside = device(ctx, x, a, b, False, q, lags, 1)
    for g in (got, inside):
        assert same_bytes(g[0], ss) and same_bytes(g[1], cs)


def test_a_nan_stays_in_its_selection():
    """A NaN coordinate gives NaN in every sum that reads the atom in that frame and in nothing else, and no fault."""
    cell = R.ORTHO
    x, _, _ = wrapped_walk(12, 6, 9, cell)
    x = np.array(x)
    x[5, 1, 2] = np.nan                                           # atom 1, frame 5
    x[7, 4, 0] = np.inf                                           # atom 4, frame 7
    q, lags = q_list(13, 2), [0, 2, 11]
    dirty_a, dirty_b, clean_a, clean_b = np.array([0, 1]), np.array([4, 5]), np.array([2, 3]), np.array([0, 3])
    exp_dirty = S.sums(x, cell, dirty_a, clean_b, False, q, lags, 1)
    exp_clean = S.sums(x, cell, clean_a, clean_b, False, q, lags, 1)
    exp_b = S.coherent_sums(x, cell, clean_a, dirty_b, q, lags, 1)
    assert np.all(np.isnan(exp_dirty[0][1].real)) and np.all(exp_dirty[0][0] == 24.0) and np.all(np.isfinite(exp_dirty[0][2].real))
    assert np.all(np.isnan(exp_dirty[1][:2].real)) and np.all(np.isfinite(exp_dirty[1][2].real))     # lag 11: origin 0 alone
    assert np.all(np.isfinite(exp_clean[0].real)) and np.all(np.isfinite(exp_clean[1].real)) and np.all(np.isnan(exp_b[:2].real))
    with Context(cell) as ctx:
        got_dirty = device(ctx, x, dirty_a, clean_b, False, q, lags, 1)
        got_clean = device(ctx, x, clean_a, clean_b, False, q, lags, 1)
        got_b = device(ctx, x, clean_a, dirty_b, False, q, lags, 1)
    assert same_but_nan(got_dirty[0], exp_dirty[0]) and same_but_nan(got_dirty[1], exp_dirty[1])
    assert same_bytes(got_clean[0], exp_clean[0]) and same_bytes(got_clean[1], exp_clean[1])
    assert same_bytes(got_b[0], exp_clean[0]) and same_but_nan(got_b[1], exp_b)      # the self part does not read list b


def test_limits_are_errors_not_faults(crowd):
    from sitator_amd import _lib_scattering
    c = crowd
    ok = dict(a=c["a"], b=c["b"], same=False, q=c["q"], lags=c["lags"], stride=1)

    def call(ctx, x, **kw):
        args = dict(ok, **kw)
        extra = {k: args.pop(k) for k in ("self_part", "coherent_part", "workspace_bytes") if k in args}
        return device(ctx, x, args["a"], args["b"], args["same"], args["q"], args["lags"], args["stride"], **extra)

    with Context(frames=np.array(c["x"])) as ctx:
        assert same_bytes(call(ctx, None)[1], c["cs"])
        for bad in (dict(lags=[150]), dict(lags=[-1]), dict(lags=[0, 1 << 40]), dict(lags=[]), dict(stride=0), dict(stride=-3),
                    dict(q=[[33, 0, 0]]), dict(q=[[0, 0, -33]]), dict(q=[[1, 1, 1], [0, 1 << 40, 0]]), dict(q=np.zeros((0, 3), dtype=np.int64)),
                    dict(q=np.zeros(((1 << 16) + 1, 3), dtype=np.int64)), dict(a=[0, 30]), dict(b=[-1]), dict(a=[3, 1 << 40]), dict(a=[]),
                    dict(b=[]), dict(same=True), dict(self_part=False, coherent_part=False), dict(workspace_bytes=100),
                    dict(workspace_bytes=-1)):
            with pytest.raises(ValueError):
                call(ctx, None, **bad)
        with pytest.raises(ValueError):                          # F other than the resident frames'
            ctx.F += 1
            try:
                call(ctx, None)
            finally:
                ctx.F -= 1
        with pytest.raises(ValueError):                          # no frame at all
            _lib_scattering.scattering(ctx, [0], [1], [[1, 0, 0]], [0], positions=np.zeros((0, 2, 3)))
        assert same_bytes(call(ctx, None)[0], c["ss"])           # and the context still works
    with Context(c["cell"]) as ctx:
        with pytest.raises(ValueError):                          # nothing resident
            call(ctx, None)


def test_a_degenerate_cell_is_refused():
    from sitator_amd import IntermediateScattering
    traj = R.random_walk(20, 2, seed=61)
    flat = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]])
    for cell in (flat, np.zeros((3, 3))):
        with pytest.raises(ValueError):                          # numpy's inverse refuses it, or sit_scattering does
            IntermediateScattering([[1, 0, 0]], [0, 1]).compute(traj, cell, [0, 1])


def test_operators_on_the_frames_an_analysis_left_resident():
    from sitator_amd import IntermediateScattering, ScatteringResult, StructureFactor, StructureFactorResult, q_vectors
    from tests.test_gpu_vanhove import analysis
    la, frames, cell, sm, mm = analysis()
    F = len(frames)
    mobile, static = np.where(mm)[0], np.where(sm)[0]
    q = q_vectors(cell, 2.2 * 2.0 * np.pi / np.linalg.norm(cell, axis=1).max())
    assert 8 <= len(q) <= 200
    lags = [0, 1, 10, 100]
    ss, cs = S.sums(frames, cell, mobile, mobile, True, q, np.array(lags), 2)
    op = IntermediateScattering(q, lags, origin_stride=2)
    version = la._ctx.labels_version
    got = op.compute_for_analysis(la)
    assert isinstance(got, ScatteringResult)
    origins = np.array([S.n_origins(F, t, 2) for t in lags])
    n = len(mobile)
    for r in (got, op.compute(frames, cell, mm), op.compute_for_analysis(la, mask=mm), op.compute_for_analysis(la, mask=mobile)):
        assert same_bytes(r.self_sums, ss) and same_bytes(r.coherent_sums, cs)
    assert np.array_equal(got.n_origins, origins) and np.array_equal(got.lags, lags) and np.array_equal(got.q_int, q)
    recip = 2.0 * np.pi * np.linalg.inv(cell.T)
    np.testing.assert_allclose(got.q, q @ recip, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(got.q_norm, np.linalg.norm(q @ recip, axis=1), rtol=1e-14)
    assert np.array_equal(got.self, ss / (origins[:, None] * float(n))) and np.all(got.self[0] == 1.0)
    assert np.array_equal(got.coherent, cs / (origins[:, None] * np.sqrt(float(n) * float(n))))
    assert np.array_equal(got.distinct, got.coherent - got.self)
    assert np.all(np.abs(got.self) <= 1.0 + 1e-12) and np.abs(got.self[3]).min() < 0.99          # the ions moved
    edges = np.linspace(0.0, got.q_norm.max() * 1.0001, 4)
    sa, ca, da, count = got.shell_average(edges)
    which = np.searchsorted(edges, got.q_norm, "right") - 1
    assert count.sum() == len(q) and np.array_equal(count, np.bincount(which, minlength=3))
    for k in range(3):
        if count[k]:
            np.testing.assert_allclose(sa[:, k], got.self[:, which == k].mean(axis=1), rtol=1e-14)
            np.testing.assert_allclose(ca[:, k], got.coherent[:, which == k].mean(axis=1), rtol=1e-14)
            np.testing.assert_allclose(da[:, k], got.distinct[:, which == k].mean(axis=1), rtol=1e-13, atol=1e-13)
    # two selections: no self part, no distinct part; the structure factor of the ions and the ion-framework partial
    with pytest.raises(ValueError, match="self part"):
        op.compute_for_analysis(la, mask_b=sm)
    ms = IntermediateScattering(q, [0, 5], self_part=False).compute_for_analysis(la, mask_b=sm)
    exp_ms = S.coherent_sums(frames, cell, mobile, static, q, [0, 5], 1)
    assert ms.self is None and ms.distinct is None and ms.self_sums is None and same_bytes(ms.coherent_sums, exp_ms)
    assert np.array_equal(ms.coherent, exp_ms / (np.array([F, F - 5])[:, None] * np.sqrt(float(n) * float(len(static)))))
    sf = StructureFactor(q, frame_stride=3)
    s_mm = sf.compute_for_analysis(la)
    exp_mm = S.coherent_sums(frames, cell, mobile, None, q, [0], 3)[0]
    assert isinstance(s_mm, StructureFactorResult) and same_bytes(s_mm.sums, exp_mm) and s_mm.n_origins == S.n_origins(F, 0, 3)
    assert s_mm.S.dtype == np.float64 and np.array_equal(s_mm.S, (exp_mm / (s_mm.n_origins * float(n))).real) and np.all(s_mm.S >= 0.0)
    partial = sf.compute_for_analysis(la, mask_b="static")
    exp_p = S.coherent_sums(frames, cell, mobile, static, q, [0], 3)[0]
    assert same_bytes(partial.sums, exp_p) and partial.S.dtype == np.complex128
    assert np.array_equal(partial.S, exp_p / (partial.n_origins * np.sqrt(float(n) * float(len(static)))))
    assert same_bytes(sf.compute(frames, cell, mm, sm).sums, exp_p)
    mean, cnt = partial.shell_average(edges)
    assert np.array_equal(cnt, count) and mean.shape == (3,)
    with pytest.raises(ValueError):
        sf.compute_for_analysis(la, mask_b="mobile")
    with pytest.raises(IndexError):
        op.compute_for_analysis(la, mask=[frames.shape[1]])
    with pytest.raises(ValueError, match="Buffer dtype mismatch"):
        op.compute(frames.astype(np.float32), cell, mm)
    with pytest.raises(ValueError):
        IntermediateScattering([[33, 0, 0]], [0]).compute_for_analysis(la)
    assert la._ctx.labels_version == version and np.array_equal(resident_frames(la._ctx), frames)


def test_operators_refuse_frame_shards():
    from sitator_amd import IntermediateScattering, LandmarkAnalysis, SiteNetwork, Structure, StructureFactor
    c = G.Case("c1_hex_scgrid")
    sn = SiteNetwork(Structure(c.ref_positions, c.cell), c.static_mask, c.mobile_mask)
    sn.centers = c.centers
    sn.vertices = c.vertices
    la = LandmarkAnalysis(verbose=False, devices=[0, 0], **c.kwargs("dotprod"))
    la.run(sn, np.ascontiguousarray(c.frames))
    with pytest.raises(NotImplementedError):
        IntermediateScattering([[1, 0, 0]], [0, 1]).compute_for_analysis(la)
    with pytest.raises(NotImplementedError):
        StructureFactor([[1, 0, 0]]).compute_for_analysis(la)
