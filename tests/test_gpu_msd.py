"""GPU: ``sit_msd`` (msd.hip: the unwrapping, the image sums, the series, the windowed term, the autocorrelation through the
pass kernel of spectrum.hip, the direct sums) and ``MeanSquaredDisplacement`` on top of it, against the numpy restatement of
tests/msd_ref.py (itself pinned to closed forms by tests/test_msd_ref.py and to msd_plan.h by tests/test_msd_plan.py).

Inputs are random walks with Gaussian steps of sigma 0.05 from fixed seeds, some with a drift, wrapped into cells whose heights
are at least 3; every test first asserts, from the restatement alone, that no step comes within a quarter of a cell vector of the
half-way point (``max_residual < 0.25``).  Tolerances, none of them taken from what the device gives:

* images: equal to ``floor(frac[t]) - floor(frac[0])`` of the walk before it was wrapped; ``max_residual``: bit-equal to the
  restatement (the same operations in the same order; a maximum has no order).
* direct path: ``msd`` and ``r4`` within rtol 1e-12 of the ``np.longdouble`` sums (sums of non-negative terms: a float64 sum in
  another order is within 4e-16 of them); lag 0 exactly 0.
* all-lag path, per series: ``|msd_dev(tau) - msd_ref(tau)| (F - tau) <= 1e-13 sum_t y[t]^2`` against the long-double sums.  The
  numpy emulation of this algorithm class (``msd_ref.msd_fft_emulation``: zero-padded float64 transform, prefix sums of the squares
  in the order of msd_plan.h) gives at most 1.7e-15 in these units over the lengths tested here, with and without drift (2 to
  20 000 frames; run on the host); a wrong index, twiddle or window lands many orders above the bound.
* both paths on the device at the same lags: within the sum of the two bounds.
* whatever must not depend on the batch, on the other atoms or on where the positions come from: bit-equal."""
import logging

import numpy as np
import pytest

from tests import golden_util as G
from tests import msd_ref as R
from tests.test_gpu_vibfreq import resident_frames

pytestmark = pytest.mark.gpu

FFT_TOL = 1e-13
DIRECT_RTOL = 1e-12
DRIFT = (0.01, -0.008, 0.006)


class Context(object):
    """A context under ``cell`` (closed on exit).  ``frames``: made resident the way ``LandmarkAnalysis.run`` does it - the
    smallest synthetic basis first, then the frames, whose leading atoms stand for the basis' static ones; the cell is then
    that basis' (``Context.resident_cell()``)."""

    def __init__(self, cell=None, frames=None):
        self.cell, self.frames = cell, frames

    @staticmethod
    def resident_cell():
        from sitator_amd import synth
        return np.asarray(synth.config_host("C1").cell, dtype=np.float64)

    def __enter__(self):
        from sitator_amd import _lib, synth
        if self.frames is None:
            self.ctx = _lib.HipContext(np.eye(3) if self.cell is None else self.cell)
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


def wrapped_walk(F, n, seed, cell, drift=None):
    """``(wrapped positions, floors of the walk's fractional coordinates, restatement's (x_u, images, max_residual))``; the
    restatement alone says that the input can be unwrapped."""
    walk = R.random_walk(F, n, seed, drift=drift)
    wrapped, fl = R.wrap_into(walk, cell)
    ref = R.unwrap(wrapped, cell)
    assert ref[2] < 0.25
    return wrapped, fl, ref


def check_all_lags(y, got, label=""):
    """``got [n, 3, n_lags]`` (lags 0 ..) against the long-double sums of ``y [n, 3, F]``, per series."""
    n, _, F = y.shape
    lags = np.arange(got.shape[2])
    ref, _ = R.msd_direct(y, lags)
    unit = R.sum_squares(y)
    err = np.max(np.abs(got - ref) * (F - lags), axis=2) / unit
    print("%sF=%d: all-lag error %.3g of sum y^2 (bound %g)" % (label, F, float(err.max()), FFT_TOL))
    assert np.all(got[:, :, 0] == 0.0)
    assert np.all(err <= FFT_TOL)
    return ref


def check_direct(y, lags, got, got4):
    ref, ref4 = R.msd_direct(y, lags)
    moving = np.asarray(lags) > 0
    rel = np.max(np.abs(got[:, :, moving] - ref[:, :, moving]) / ref[:, :, moving]) if moving.any() else 0.0
    rel4 = np.max(np.abs(got4[:, moving] - ref4[:, moving]) / ref4[:, moving]) if moving.any() else 0.0
    print("F=%d: direct rel error msd %.3g, r4 %.3g (bound %g)" % (y.shape[2], float(rel), float(rel4), DIRECT_RTOL))
    assert np.all(got[:, :, ~moving] == 0.0) and np.all(got4[:, ~moving] == 0.0)
    assert rel <= DIRECT_RTOL and rel4 <= DIRECT_RTOL
    return ref


# ---- 1. the unwrapping ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.CELLS))
def test_images_are_the_floors_of_the_walk(name):
    cell = R.CELLS[name]
    F, n = 700, 35                                               # more than one tile of atoms, a ragged tile of frames
    wrapped, fl, (xu, images_ref, res_ref) = wrapped_walk(F, n, 3, cell, drift=DRIFT)
    expect = (fl - fl[:1]).transpose(1, 0, 2)
    assert np.abs(expect).max() >= 2 and np.array_equal(images_ref, expect)
    with Context(cell) as ctx:
        msd, _, _, images, res = ctx.msd(positions=wrapped, max_lag=8, images=True)
    assert images.dtype == np.int32 and np.array_equal(images, expect)
    assert res == res_ref and 0.0 < res < 0.25
    check_all_lags(R.series(wrapped, cell), msd)


def test_an_unwrapped_walk_passes_through():
    """All images 0; the series is x[t] - x[0] bit for bit: what comes out is what comes out without unwrapping."""
    cell = R.TRICLINIC
    walk = R.random_walk(300, 4, seed=4, drift=DRIFT)
    xu, images_ref, res_ref = R.unwrap(walk, cell)
    assert res_ref < 0.25 and not images_ref.any() and np.array_equal(xu, walk)
    assert np.abs(R.fractional(walk, cell)).max() > 2            # it does leave the cell
    lags = [0, 1, 5, 150, 299]
    with Context(cell) as ctx:
        a = ctx.msd(positions=walk, max_lag=299, images=True)
        b = ctx.msd(positions=walk, max_lag=299, unwrap=False, images=True)
        c = ctx.msd(positions=walk, lags=lags, r4=True)
        d = ctx.msd(positions=walk, lags=lags, r4=True, unwrap=False)
    assert not a[3].any() and not b[3].any()
    assert np.array_equal(a[0], b[0]) and np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1])
    assert a[4] == res_ref == c[4] and b[4] == 0.0 and d[4] == 0.0
    check_direct(R.series(walk), lags, c[0], c[1])


# ---- 2. the direct path -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [2, 3, 5, 33, 257, 1000])
def test_direct_lags(F):
    cell = R.HEX
    wrapped, _, _ = wrapped_walk(F, 3, 10 + F, cell, drift=DRIFT)
    lags = np.clip([0, 1, 2, F // 2, F - 2, F - 1], 0, F - 1)    # duplicates at the smallest lengths: allowed
    y = R.series(wrapped, cell)
    with Context(cell) as ctx:
        msd, r4, _, _, _ = ctx.msd(positions=wrapped, lags=lags, r4=True)
    check_direct(y, lags, msd, r4)


# ---- 3. the all-lag path ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [2, 3, 4, 5, 33, 511, 512, 513, 1000, 4099, 20000])
def test_all_lags(F):
    cell = R.TRICLINIC
    n = 2 if F <= 1000 else 1
    wrapped, _, _ = wrapped_walk(F, n, 20 + F, cell, drift=DRIFT if F % 2 else None)
    y = R.series(wrapped, cell)
    with Context(cell) as ctx:
        msd = ctx.msd(positions=wrapped, max_lag=F - 1)[0]
        half = ctx.msd(positions=wrapped)[0]                     # the default: lags 0 .. F // 2, the same numbers
        assert half.shape[2] == F // 2 + 1 and np.array_equal(half, msd[:, :, :F // 2 + 1])
        ref = check_all_lags(y, msd)
        if F == 1000:                                            # the two paths of the device against each other
            lags = np.array([0, 1, 2, 500, 998, 999])
            direct = ctx.msd(positions=wrapped, lags=lags)[0]
            bound = FFT_TOL * np.asarray(R.sum_squares(y), dtype=np.float64)[:, :, None] / (F - lags) \
                + DIRECT_RTOL * np.asarray(ref[:, :, lags], dtype=np.float64)
            assert np.all(np.abs(direct - msd[:, :, lags]) <= bound)


@pytest.mark.parametrize("F,bits", [(700, 4), (100, 3), (33, 3), (5, 2)])
def test_three_passes_at_small_lengths(monkeypatch, F, bits):
    """SITATOR_SPECTRUM_STAGE_BITS shortens the passes: the three-pass chain at lengths one can follow by hand."""
    monkeypatch.setenv("SITATOR_SPECTRUM_STAGE_BITS", str(bits))
    cell = R.ORTHO
    wrapped, _, _ = wrapped_walk(F, 3, F, cell, drift=DRIFT)
    with Context(cell) as ctx:
        msd = ctx.msd(positions=wrapped, max_lag=F - 1)[0]
    check_all_lags(R.series(wrapped, cell), msd)


def test_smallest_length_of_three_passes():
    F = 524289
    cell = R.TRICLINIC
    wrapped, _, _ = wrapped_walk(F, 1, 9, cell)
    y = R.series(wrapped, cell)
    lags = np.unique(np.concatenate([[0, 1, 2, F // 2, F - 2, F - 1], np.random.default_rng(1).integers(0, F, size=44)]))
    with Context(cell) as ctx:
        msd = ctx.msd(positions=wrapped, max_lag=F - 1)[0]
    ref, _ = R.msd_direct(y, lags)
    err = np.max(np.abs(msd[:, :, lags] - ref) * (F - lags), axis=2) / R.sum_squares(y)
    print("F=%d: all-lag error %.3g of sum y^2 at %d lags (bound %g)" % (F, float(err.max()), len(lags), FFT_TOL))
    assert msd[0, 0, 0] == 0.0 and np.all(err <= FFT_TOL)


# ---- 4. batching and independence -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crowd():
    """F = 257, 140 atoms wrapped into the cell resident frames come with; ``order``: a fixed shuffle of the atoms."""
    cell = Context.resident_cell()
    assert np.all(R.heights(cell) >= 3.0)
    wrapped, _, _ = wrapped_walk(257, 140, 21, cell, drift=DRIFT)
    wrapped.flags.writeable = False
    return cell, wrapped, np.random.default_rng(22).permutation(140)


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("direct", [False, True], ids=["all_lags", "direct"])
def test_batches_and_neighbours_do_not_change_an_atom(crowd, direct):
    cell, traj, _ = crowd
    sel = [3, 17, 40, 41, 99]
    pos = np.ascontiguousarray(traj[:, sel])
    kw = dict(lags=[0, 1, 2, 128, 255, 256], r4=True) if direct else dict(max_lag=256)
    n_lags = 6 if direct else 257
    ab, fixed = R.atom_bytes(257, n_lags, direct), R.fixed_bytes(257, True)
    with Context(cell) as ctx:
        whole = ctx.msd(positions=pos, collective=True, images=True, **kw)
        for cap in (fixed + ab, fixed + 2 * ab + 100):           # batches of one; of two with a ragged last one
            assert same(whole, ctx.msd(positions=pos, collective=True, images=True, workspace_bytes=cap, **kw))
        for i in range(len(sel)):
            alone = ctx.msd(positions=np.ascontiguousarray(pos[:, i:i + 1]), images=True, **kw)
            assert np.array_equal(whole[0][i:i + 1], alone[0]) and np.array_equal(whole[3][i:i + 1], alone[3])
            if direct:
                assert np.array_equal(whole[1][i:i + 1], alone[1])
        with pytest.raises(ValueError):
            ctx.msd(positions=pos, collective=True, workspace_bytes=fixed + ab - 256, **kw)
        with pytest.raises(ValueError):
            ctx.msd(positions=pos, workspace_bytes=ab - 256, **kw)
        assert same(whole[:2], ctx.msd(positions=pos, workspace_bytes=ab, **kw)[:2])


@pytest.mark.parametrize("n_sel", [1, 3, 31, 32, 33, 65])             # 31, 32, 33: the edges of the tile across the atoms
def test_resident_frames_and_an_atom_list(crowd, n_sel):
    """An atom's result from a host array and from the resident frames with an atom list that is not contiguous, the
    atoms that are not selected holding NaN: bit-equal, and the context stays as it was."""
    cell, traj, order = crowd
    sel = np.sort(order[:n_sel])
    mask = np.zeros(140, dtype=bool)
    mask[sel] = True
    holed = np.where(mask[None, :, None], traj, np.nan)
    y = R.series(np.ascontiguousarray(traj[:, sel]), cell)
    lags = [0, 1, 100, 256]
    with Context(frames=holed) as ctx:
        version = ctx.labels_version
        host = ctx.msd(positions=np.ascontiguousarray(holed[:, sel]), max_lag=256, collective=True, images=True)
        check_all_lags(y, host[0])
        res = ctx.msd(atoms=sel, max_lag=256, collective=True, images=True)
        assert same(host, res) and host[4] == res[4]
        assert same(ctx.msd(positions=np.ascontiguousarray(holed[:, sel]), lags=lags, r4=True), ctx.msd(atoms=sel, lags=lags, r4=True))
        assert ctx.labels_version == version
        assert np.array_equal(resident_frames(ctx), holed, equal_nan=True)


def bitwise(a, b):
    return all((x is None and y is None) or (x.shape == y.shape and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


@pytest.mark.parametrize("F", [2, 33, 34])
def test_an_atom_list_in_any_order(F):
    """Resident frames and an atom list that descends and names one atom twice - 5 columns out of 40, the others holding
    NaN - at the edges of the tile along the frames: bit for bit what the host array ``traj[:, list]`` gives, on both
    paths, and the images are the restatement's."""
    cell = Context.resident_cell()
    wrapped, _, _ = wrapped_walk(F, 40, 80 + F, cell, drift=DRIFT)
    sel = np.array([37, 30, 30, 12, 3])
    mask = np.zeros(40, dtype=bool)
    mask[sel] = True
    holed = np.where(mask[None, :, None], wrapped, np.nan)
    pos = np.ascontiguousarray(holed[:, sel])
    _, images_ref, res_ref = R.unwrap(pos, cell)
    lags = [0, 1, F - 1]
    with Context(frames=holed) as ctx:
        host = ctx.msd(positions=pos, max_lag=F - 1, collective=True, images=True)
        res = ctx.msd(atoms=sel, max_lag=F - 1, collective=True, images=True)
        host_d = ctx.msd(positions=pos, lags=lags, r4=True, collective=True, images=True)
        res_d = ctx.msd(atoms=sel, lags=lags, r4=True, collective=True, images=True)
    assert bitwise(host[:4], res[:4]) and host[4] == res[4] == res_ref
    assert bitwise(host_d[:4], res_d[:4]) and host_d[4] == res_d[4] == res_ref
    assert np.array_equal(res[3], images_ref) and np.array_equal(res_d[3], images_ref)
    assert res[0][1].tobytes() == res[0][2].tobytes() and np.all(np.isfinite(res[0])) and np.all(np.isfinite(res[2]))
    check_all_lags(R.series(pos, cell), res[0])


@pytest.mark.parametrize("F", [33, 1025])
def test_spectrum_and_msd_take_turns_on_one_context(F):
    """The two operators share the pass kernel's table of roots and pad to different lengths here (64 and 128 points at
    F = 33, 2048 and 4096 at F = 1025): a spectrum after an MSD is the spectrum before it, bit for bit, and each is right."""
    from tests import vibfreq_ref as V
    from tests.test_gpu_vibfreq import check_against_numpy
    traj = R.random_walk(F, 3, seed=90 + F)
    freqs, fmask = V.band(F - 1)
    with Context(R.TRICLINIC) as ctx:
        first = ctx.speed_spectrum(freqs, fmask, positions=traj, spectrum=True, speeds=True)
        msd = ctx.msd(positions=traj, max_lag=F - 1)
        third = ctx.speed_spectrum(freqs, fmask, positions=traj, spectrum=True, speeds=True)
        again = ctx.msd(positions=traj, max_lag=F - 1)
    assert bitwise(first, third) and bitwise(msd[:1], again[:1])
    check_against_numpy(V.restatement(traj, slice(None)), *first)
    check_all_lags(R.series(traj, R.TRICLINIC), msd[0])


def test_nan_stays_with_its_atom(crowd):
    cell, traj, _ = crowd
    t = np.array(traj[:, :4])
    t[100, 2, 1] = np.nan
    t[7, 2, 0] = np.inf
    keep = [0, 1, 3]
    with Context(cell) as ctx:
        clean = ctx.msd(positions=np.ascontiguousarray(traj[:, keep]), max_lag=256, images=True)
        dirty = ctx.msd(positions=t, max_lag=256, images=True)
        clean_d = ctx.msd(positions=np.ascontiguousarray(traj[:, keep]), lags=[0, 3, 50], r4=True)
        dirty_d = ctx.msd(positions=t, lags=[0, 3, 50], r4=True)
    assert np.array_equal(dirty[0][keep], clean[0]) and np.array_equal(dirty[3][keep], clean[3])
    assert np.array_equal(dirty_d[0][keep], clean_d[0]) and np.array_equal(dirty_d[1][keep], clean_d[1])
    assert dirty[4] == R.unwrap(t, cell)[2] and 0.0 < dirty[4] < 0.25        # the maximum is over the finite steps
    assert np.all(dirty[0][2, :, 0] == 0.0) and np.all(np.isnan(dirty[0][2, 1, 1:]))
    assert np.all(np.isnan(dirty_d[0][2, 1, 1:])) and np.all(np.isnan(dirty_d[1][2, 1:]))


# ---- 5. the collective displacement -------------------------------------------------------------------------------------

def test_collective():
    cell = R.HEX
    F = 600
    wrapped, _, _ = wrapped_walk(F, 4, 51, cell, drift=DRIFT)
    y = R.series(wrapped, cell)
    Y = R.collective_series(y)
    lags = [0, 1, 2, 300, 598, 599]
    with Context(cell) as ctx:
        msd, _, coll, _, _ = ctx.msd(positions=wrapped, max_lag=F - 1, collective=True)
        one = ctx.msd(positions=np.ascontiguousarray(wrapped[:, 2:3]), max_lag=F - 1, collective=True)
        direct = ctx.msd(positions=wrapped, lags=lags, collective=True)
        one_d = ctx.msd(positions=np.ascontiguousarray(wrapped[:, 2:3]), lags=lags, collective=True)
        # two atoms that move oppositely (no unwrapping: the second is the first negated, exactly): Y is zero
        walk = R.random_walk(F, 1, seed=52)
        pair = np.ascontiguousarray(np.concatenate([walk, -walk], axis=1))
        opposite = ctx.msd(positions=pair, max_lag=F - 1, collective=True, unwrap=False)
        opposite_d = ctx.msd(positions=pair, lags=lags, collective=True, unwrap=False)
    assert coll.shape == (3, F)
    check_all_lags(Y, coll[None] * 4.0, "collective ")           # the MSD of Y, divided by n_sel = 4 (a power of two: exact)
    check_direct(Y, lags, direct[2][None] * 4.0, np.zeros((1, len(lags))) + np.asarray(R.msd_direct(Y, lags)[1], dtype=np.float64))
    assert np.array_equal(one[2], one[0][0]) and np.array_equal(one_d[2], one_d[0][0])    # one atom: the tracer result
    assert np.array_equal(msd[2], one[0][0])
    # Y = 0 for the pair; the bound is that of its two series, whose sum it is
    unit = np.asarray(R.sum_squares(R.series(pair)), dtype=np.float64)[0]
    assert np.all(np.abs(opposite[2]) * (F - np.arange(F)) <= FFT_TOL * unit[:, None])
    assert np.all(opposite_d[2] == 0.0)


# ---- 6. limits ------------------------------------------------------------------------------------------------------------

def test_limits_are_errors_not_faults(crowd):
    cell, traj, _ = crowd
    pos = np.ascontiguousarray(traj[:, :3])
    with Context(frames=np.array(traj)) as ctx:
        for bad in ([0, 140], [-1], [3, 1 << 40]):
            with pytest.raises((ValueError, IndexError)):
                ctx.msd(atoms=bad)
        assert np.isfinite(ctx.msd(atoms=[139])[0]).all()
        for bad in ([257], [-1], [0, 1, 1 << 40]):
            with pytest.raises((ValueError, IndexError)):
                ctx.msd(atoms=[5], lags=bad)
        for bad in (257, -1, 1 << 40):
            with pytest.raises((ValueError, IndexError)):
                ctx.msd(atoms=[5], max_lag=bad)
        assert ctx.msd(atoms=[5], max_lag=256)[0].shape == (1, 3, 257)
        with pytest.raises(ValueError):                          # F other than the resident frames'
            ctx.F += 1
            try:
                ctx.msd(atoms=[5])
            finally:
                ctx.F -= 1
        with pytest.raises(ValueError):                          # one frame: no displacement
            ctx.msd(positions=np.zeros((1, 2, 3)), max_lag=0)
        with pytest.raises(ValueError):                          # the fourth moment needs a lag list
            ctx.msd(positions=pos, r4=True)
        with pytest.raises(ValueError):
            ctx.msd(positions=pos, workspace_bytes=1024)
        assert ctx.msd(positions=np.zeros((5, 0, 3)))[0].shape == (0, 3, 3)
    with Context(cell) as ctx:
        with pytest.raises(ValueError):                          # nothing resident
            ctx.msd(atoms=[0])


def test_a_degenerate_cell_cannot_unwrap():
    from sitator_amd import MeanSquaredDisplacement
    traj = R.random_walk(20, 2, seed=61)
    flat = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]])     # determinant 0, exactly, in integers
    with pytest.raises(ValueError):                              # numpy's inverse refuses it, or sit_msd does
        MeanSquaredDisplacement().compute(traj, flat, [0, 1])
    with pytest.raises(ValueError):
        MeanSquaredDisplacement().compute(traj, np.zeros((3, 3)), [0, 1])
    out = MeanSquaredDisplacement(unwrap=False).compute(traj, flat, [0, 1])  # no unwrapping: the cell is not looked at
    check_all_lags(R.series(traj), np.ascontiguousarray(out.msd_axes.transpose(0, 2, 1)))


# ---- 7. the operator ------------------------------------------------------------------------------------------------------

def test_operator_result_and_warning(caplog):
    from sitator_amd import MeanSquaredDisplacement, MSDResult
    cell = R.TRICLINIC
    F = 400
    wrapped, fl, (_, images_ref, res_ref) = wrapped_walk(F, 5, 71, cell, drift=DRIFT)
    keep = wrapped.copy()
    mask = np.array([True, False, True, True, False])
    y = R.series(np.ascontiguousarray(wrapped[:, mask]), cell)
    with caplog.at_level(logging.WARNING, logger="sitator_amd.dynamics"):
        res = MeanSquaredDisplacement(collective=True).compute(wrapped, cell, mask, images=True)
    assert not caplog.records
    assert isinstance(res, MSDResult) and np.array_equal(wrapped, keep)
    assert np.array_equal(res.lags, np.arange(F // 2 + 1)) and res.msd_axes.shape == (3, F // 2 + 1, 3)
    check_all_lags(y, np.ascontiguousarray(res.msd_axes.transpose(0, 2, 1)))
    assert np.array_equal(res.msd, (res.msd_axes[..., 0] + res.msd_axes[..., 1]) + res.msd_axes[..., 2])
    assert np.array_equal(res.mean, np.mean(res.msd, axis=0)) and res.collective.shape == (F // 2 + 1, 3)
    assert res.alpha2 is None and np.array_equal(res.images, images_ref[mask])
    assert res.max_residual == R.unwrap(np.ascontiguousarray(wrapped[:, mask]), cell)[2]
    b = MeanSquaredDisplacement(collective=True).compute(wrapped, cell, np.where(mask)[0])
    assert np.array_equal(b.msd_axes, res.msd_axes) and b.images is None
    # explicit lags: the non-Gaussian parameter from the fourth moment
    lags = [0, 1, 4, 16, 64, 256]
    d = MeanSquaredDisplacement(lags=lags).compute(wrapped, cell, mask)
    ref, ref4 = R.msd_direct(y, lags)
    check_direct(y, lags, np.ascontiguousarray(d.msd_axes.transpose(0, 2, 1)), d.r4)
    tot = np.asarray(np.sum(ref, axis=1), dtype=np.float64)
    np.testing.assert_allclose(d.alpha2[:, 1:], 3.0 * np.asarray(ref4, dtype=np.float64)[:, 1:] / (5.0 * tot[:, 1:] ** 2) - 1.0,
                               rtol=0, atol=1e-11)               # 3 r4 / (5 msd^2) is of order 1: three factors within 1e-12
    assert np.array_equal(d.lags, lags) and d.collective is None and np.all(np.isnan(d.alpha2[:, 0]))
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'double' but got 'float32'"):
        MeanSquaredDisplacement().compute(wrapped.astype(np.float32), cell, mask)
    with pytest.raises(ValueError):
        MeanSquaredDisplacement(max_lag=3, lags=[1])
    # steps of 0.3 cell vectors: one warning
    jumpy = (np.arange(12)[:, None, None] * 0.3 * cell[0][None, None, :]) + np.zeros((12, 2, 3))
    with caplog.at_level(logging.WARNING, logger="sitator_amd.dynamics"):
        r = MeanSquaredDisplacement().compute(jumpy, cell, [0, 1])
    assert len(caplog.records) == 1 and 0.25 < r.max_residual <= 0.5


def test_operator_on_the_frames_an_analysis_left_resident():
    from sitator_amd import MeanSquaredDisplacement, LandmarkAnalysis, SiteNetwork, Structure
    c = G.Case("c1_hex_scgrid")
    sn = SiteNetwork(Structure(c.ref_positions, c.cell), c.static_mask, c.mobile_mask)
    sn.centers = c.centers
    sn.vertices = c.vertices
    frames = np.ascontiguousarray(c.frames)
    la = LandmarkAnalysis(verbose=False, **c.kwargs("dotprod"))
    op = MeanSquaredDisplacement(collective=True)
    with pytest.raises(ValueError):
        op.compute_for_analysis(la)                                                      # has not run
    st = la.run(sn, frames)
    version = la._ctx.labels_version
    exp = op.compute(frames, c.cell, c.mobile_mask, images=True)
    for got in (op.compute_for_analysis(la, images=True), op.compute_for_analysis(la, mask=c.mobile_mask, images=True),
                op.compute_for_analysis(la, mask=np.where(c.mobile_mask)[0], images=True)):
        for name in ("lags", "msd_axes", "msd", "mean", "collective", "images"):
            assert np.array_equal(getattr(got, name), getattr(exp, name)), name          # bit-equal
        assert got.max_residual == exp.max_residual and got.alpha2 is None
    d = MeanSquaredDisplacement(lags=[0, 1, 10]).compute_for_analysis(la, mask=c.static_mask)
    e = MeanSquaredDisplacement(lags=[0, 1, 10]).compute(frames, c.cell, c.static_mask)
    assert np.array_equal(d.msd_axes, e.msd_axes) and np.array_equal(d.alpha2, e.alpha2, equal_nan=True)
    with pytest.raises(IndexError):
        op.compute_for_analysis(la, mask=[frames.shape[1]])
    assert la._ctx.labels_version == version
    assert np.array_equal(st.traj, c.out("dotprod")["labels"])
    assert np.array_equal(resident_frames(la._ctx), frames)


def test_operator_accepts_frames_recentred_on_the_device():
    from sitator_amd import MeanSquaredDisplacement, LandmarkAnalysis, RecenterTrajectory, SiteNetwork, Structure, synth
    host = synth.config_host("C1b")
    frames, sm, mm, ref = synth.make_trajectory(host, 4, 400, seed=31, p_hop=1.0 / 50)
    frames = frames + np.cumsum(np.random.default_rng(3).normal(scale=0.002, size=(len(frames), 1, 3)), axis=0)
    masses = np.random.default_rng(4).uniform(1.0, 40.0, size=frames.shape[1])
    ref_rec = ref[None].copy()
    RecenterTrajectory().run(Structure(ref, host.cell), sm, ref_rec, masses=masses)   # the basis recentred the same way
    sn = SiteNetwork(Structure(ref_rec[0], host.cell), sm, mm)
    sn.centers = np.asarray(host.centers) + (ref_rec[0, 0] - ref[0])
    sn.vertices = host.vertices
    la = LandmarkAnalysis(verbose=False, recenter_masses=masses)
    la.run(sn, frames)
    got = MeanSquaredDisplacement(max_lag=50).compute_for_analysis(la)
    # the frames on the device are the recentred ones: the same operator on them as a host array
    exp = MeanSquaredDisplacement(max_lag=50).compute(resident_frames(la._ctx), host.cell, mm)
    assert np.array_equal(got.msd_axes, exp.msd_axes) and np.all(np.isfinite(got.msd))


def test_operator_refuses_frame_shards():
    from sitator_amd import MeanSquaredDisplacement, LandmarkAnalysis, SiteNetwork, Structure
    c = G.Case("c1_hex_scgrid")
    sn = SiteNetwork(Structure(c.ref_positions, c.cell), c.static_mask, c.mobile_mask)
    sn.centers = c.centers
    sn.vertices = c.vertices
    la = LandmarkAnalysis(verbose=False, devices=[0, 0], **c.kwargs("dotprod"))
    la.run(sn, np.ascontiguousarray(c.frames))
    with pytest.raises(NotImplementedError):
        MeanSquaredDisplacement().compute_for_analysis(la)


def test_diffusion_coefficient():
    from sitator_amd import diffusion_coefficient
    D, c = 0.0123, 0.4
    t = np.arange(1, 300)
    got, icpt = diffusion_coefficient(t, 6 * D * t + c)
    np.testing.assert_allclose(got, D, rtol=1e-12)
    np.testing.assert_allclose(icpt, c, rtol=1e-9)
