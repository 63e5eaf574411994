"""GPU: ``sit_speed_spectrum`` (spectrum.hip: the speeds, Bluestein's transform over power-of-two passes in LDS, the band
sums) and ``AverageVibrationalFrequency`` on top of it, against numpy (``np.fft.rfft``, the restatement of
tests/vibfreq_ref.py) and against what the reference's class returned (tests/golden/vibfreq_known_answers.npz).

Inputs are random walks with Gaussian steps of sigma 0.05 from fixed seeds.  Tolerances, none of them taken from what the
device gives:

* speeds: bit-equal to numpy - the same operations in the same order, an IEEE square root.
* spectrum: ``max_k |X_dev[k] - X_np[k]| <= 1e-13 sqrt(n) ||s||_2`` per atom.  A numpy emulation of this algorithm class
  (radix-2 passes, host-made tables, integer-reduced chirp phase) stays below 1.0e-15 in these units for n from 2 to
  99 999; an indexing or twiddle mistake lands many orders above the bound.
* avg: rtol 1e-11 against the restatement (the emulation's worst case: 1.1e-14).
* whatever must not depend on the batch, on the other atoms or on where the positions come from: bit-equal.

The lengths are the smallest at which the transform can go wrong: the first bins, powers of two and primes, every step
of the padded length, one pass to two (n = 512 to 513) and two to three (n = 524 289), and an n at which a chirp phase
that is not reduced in integers shows."""
import ctypes

import numpy as np
import pytest

from tests import golden_util as G
from tests import vibfreq_ref as V

pytestmark = pytest.mark.gpu

VG = V.VibGoldens()
SPEC_TOL = 1e-13
AVG_RTOL = 1e-11


class Context(object):
    """A context (closed on exit).  ``frames``: made resident the way ``LandmarkAnalysis.run`` does it - a basis first (the
    smallest synthetic one: the spectrum looks at neither the basis nor the cell), then the frames, whose leading atoms
    stand for the basis' static ones."""

    def __init__(self, frames=None):
        self.frames = frames

    def __enter__(self):
        from sitator_amd import _lib, synth
        if self.frames is None:
            self.ctx = _lib.HipContext(np.eye(3))
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
    hip = ctx.lib                                  # the library's handle resolves the runtime it is linked against
    out = np.empty((ctx.F, ctx.A, 3))
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ctx.synchronize()
    assert hip.hipMemcpy(out.ctypes.data, ctx.frames_device_ptr(), out.nbytes, 2) == 0
    return out


def check_against_numpy(ref, avg, power, spec, speeds):
    """speeds bit-equal, every atom's bins within its own bound, avg and band power against the restatement."""
    n = ref["speeds"].shape[1]
    assert speeds.shape == ref["speeds"].shape and np.array_equal(speeds, ref["speeds"])
    assert spec.shape == ref["spectrum"].shape
    err = np.max(np.abs(spec - ref["spectrum"]), axis=1) / (np.sqrt(n) * np.linalg.norm(ref["speeds"], axis=1))
    rel = np.max(np.abs(avg - ref["avg"]) / np.abs(ref["avg"]))
    print("n=%d: spectrum error %.3g (bound %g), avg rel error %.3g (bound %g)" % (n, err.max(), SPEC_TOL, rel, AVG_RTOL))
    assert np.all(err <= SPEC_TOL)
    np.testing.assert_allclose(avg, ref["avg"], rtol=AVG_RTOL, atol=0)
    np.testing.assert_allclose(power, ref["band_power"], rtol=AVG_RTOL, atol=0)


def check_over_atoms(got, mean, std=None):
    """The operator's result.  The mean of per-atom values that are each within rtol 1e-11 is within it too; the standard
    deviation moves by at most the largest per-atom error, AVG_RTOL x the largest value - an absolute bound, since the
    deviation itself may be zero (a band of one bin)."""
    if std is None:
        np.testing.assert_allclose(got, mean, rtol=AVG_RTOL, atol=0)
    else:
        assert isinstance(got, tuple) and len(got) == 2
        np.testing.assert_allclose(got[0], mean, rtol=AVG_RTOL, atol=0)
        np.testing.assert_allclose(got[1], std, rtol=0, atol=AVG_RTOL * 0.5)       # every frequency is at most 0.5


def host_call(ctx, traj, mask, band=(0, np.inf), **kw):
    freqs, fmask = V.band(len(traj) - 1, *band)
    return ctx.speed_spectrum(freqs, fmask, positions=np.ascontiguousarray(traj[:, mask]), spectrum=True, speeds=True, **kw)


# ---- 1. lengths -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 4, 5, 31, 32, 33, 511, 512, 513, 1000, 4099, 20000])
def test_lengths(n):
    traj = V.random_walk(n + 1, 3, seed=100 + n)
    ref = V.restatement(traj, slice(None))
    with Context() as ctx:
        check_against_numpy(ref, *host_call(ctx, traj, slice(None)))


def test_smallest_length_of_three_passes():
    n = 524289
    traj = V.random_walk(n + 1, 1, seed=9)
    ref = V.restatement(traj, slice(None))
    with Context() as ctx:
        check_against_numpy(ref, *host_call(ctx, traj, slice(None)))


@pytest.mark.parametrize("n,bits", [(700, 4), (100, 3), (33, 3), (5, 2)])
def test_three_passes_at_small_lengths(monkeypatch, n, bits):
    """SITATOR_SPECTRUM_STAGE_BITS shortens the passes: the three-pass chain (two levels of twiddles) at lengths where
    every index is small enough to follow by hand."""
    monkeypatch.setenv("SITATOR_SPECTRUM_STAGE_BITS", str(bits))
    traj = V.random_walk(n + 1, 3, seed=n)
    ref = V.restatement(traj, slice(None))
    with Context() as ctx:
        check_against_numpy(ref, *host_call(ctx, traj, slice(None)))


# ---- 2. atoms -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crowd():
    """n = 257, 140 atoms; ``order``: a fixed shuffle of the atoms to select from."""
    traj = V.random_walk(258, 140, seed=21)
    traj.flags.writeable = False
    return traj, np.random.default_rng(22).permutation(140)


@pytest.mark.parametrize("n_sel", [1, 2, 3, 31, 32, 33, 65, 130])     # 31, 32, 33: the edges of the tile across the atoms
def test_atoms(crowd, n_sel):
    traj, order = crowd
    sel = np.sort(order[:n_sel])                                 # not contiguous
    mask = np.zeros(140, dtype=bool)
    mask[sel] = True
    ref = V.restatement(traj, mask)
    holed = np.where(mask[None, :, None], traj, np.nan)          # whoever is not selected holds NaN
    with Context(holed) as ctx:
        version = ctx.labels_version
        host = host_call(ctx, holed, mask)
        check_against_numpy(ref, *host)
        freqs, fmask = V.band(257)
        res = ctx.speed_spectrum(freqs, fmask, atoms=sel, spectrum=True, speeds=True)
        for a, b in zip(host, res):
            assert np.array_equal(a, b)                          # resident frames + atom list: bit-identical
        assert ctx.labels_version == version
        assert np.array_equal(resident_frames(ctx), holed, equal_nan=True)


@pytest.mark.parametrize("F", [2, 33, 34])
def test_an_atom_list_in_any_order(F):
    """Resident frames and an atom list that descends and names one atom twice - 5 columns out of 40, the others holding
    NaN - at the edges of the tile along the frames (n = 1, 32, 33): bit for bit what the host array ``traj[:, list]``
    gives, and the speeds are numpy's.  With n = 1 the band is empty: avg is 0 / 0 on either way."""
    traj = V.random_walk(F, 40, seed=60 + F)
    sel = np.array([37, 30, 30, 12, 3])
    mask = np.zeros(40, dtype=bool)
    mask[sel] = True
    holed = np.where(mask[None, :, None], traj, np.nan)
    d = traj[1:, sel] - traj[:-1, sel]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    expect = np.ascontiguousarray(np.sqrt((dx * dx + dy * dy) + dz * dz).T)
    freqs, fmask = V.band(F - 1)
    with Context(holed) as ctx:
        host = ctx.speed_spectrum(freqs, fmask, positions=np.ascontiguousarray(holed[:, sel]), spectrum=True, speeds=True)
        res = ctx.speed_spectrum(freqs, fmask, atoms=sel, spectrum=True, speeds=True)
    for a, b in zip(host, res):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert res[3].shape == (5, F - 1) and res[3].tobytes() == expect.tobytes()
    assert res[2][1].tobytes() == res[2][2].tobytes() and np.all(np.isfinite(res[2]))     # the atom named twice
    if F > 2:
        np.testing.assert_allclose(res[0], V.restatement(traj, sel)["avg"], rtol=AVG_RTOL, atol=0)


def test_nan_stays_with_its_atom(crowd):
    traj, _ = crowd
    t = np.array(traj[:, :4])
    t[100, 2, 1] = np.nan
    ref = V.restatement(traj, [0, 1, 3])
    with Context() as ctx:
        avg, power, _, _ = host_call(ctx, t, slice(None))
    assert np.isnan(avg[2]) and np.isnan(power[2]) and np.all(np.isfinite(avg[[0, 1, 3]]))
    np.testing.assert_allclose(avg[[0, 1, 3]], ref["avg"], rtol=AVG_RTOL, atol=0)


# ---- 3. batching and independence -----------------------------------------------------------------------------------

def test_batches_and_neighbours_do_not_change_an_atom(crowd):
    traj, _ = crowd
    sel = [3, 17, 40, 41, 99]
    freqs, fmask = V.band(257)
    pos = np.ascontiguousarray(traj[:, sel])
    # what one atom's transform takes, with the bins staged: the plan's own arithmetic (spectrum_plan.h)
    atom_bytes = -(-(1024 * 16 + 257 * 8 + 1 * 16 + 16 + 129 * 16) // 256) * 256     # M = 1024: one pass, one workgroup
    with Context() as ctx:
        whole = ctx.speed_spectrum(freqs, fmask, positions=pos, spectrum=True, speeds=True)
        check_against_numpy(V.restatement(traj, sel), *whole)
        for cap in (atom_bytes, 2 * atom_bytes + 100):           # batches of one; of two with a ragged last one
            part = ctx.speed_spectrum(freqs, fmask, positions=pos, spectrum=True, speeds=True, workspace_bytes=cap)
            for a, b in zip(whole, part):
                assert np.array_equal(a, b)
        for i in range(len(sel)):
            alone = ctx.speed_spectrum(freqs, fmask, positions=np.ascontiguousarray(pos[:, i:i + 1]), spectrum=True, speeds=True)
            for a, b in zip(whole, alone):
                assert np.array_equal(a[i:i + 1], b)
        with pytest.raises(ValueError):
            ctx.speed_spectrum(freqs, fmask, positions=pos, spectrum=True, workspace_bytes=atom_bytes - 256)


def test_a_quiet_atom_keeps_its_own_tolerance():
    """One walk scaled by 1e-3 among unscaled ones: its error is measured against its own ||s||_2."""
    traj = V.random_walk(1001, 4, seed=5, scale=[1.0, 1e-3, 1.0, 1.0])
    ref = V.restatement(traj, slice(None))
    assert np.linalg.norm(ref["speeds"][1]) < 2e-3 * np.linalg.norm(ref["speeds"][0])
    with Context() as ctx:
        check_against_numpy(ref, *host_call(ctx, traj, slice(None)))


# ---- 4. limits ------------------------------------------------------------------------------------------------------

def test_limits_are_errors_not_faults(crowd):
    traj, _ = crowd
    freqs, fmask = V.band(257)
    with Context(np.array(traj)) as ctx:
        for bad in ([0, 140], [-1], [3, 1 << 40]):
            with pytest.raises(ValueError):
                ctx.speed_spectrum(freqs, fmask, atoms=bad)
        ok = ctx.speed_spectrum(freqs, fmask, atoms=[139])[0]
        assert np.isfinite(ok).all()
        with pytest.raises(ValueError):                          # one frame: no speeds
            ctx.speed_spectrum(np.zeros(1), np.zeros(1, dtype=bool), positions=np.zeros((1, 2, 3)))
    with Context() as ctx:
        with pytest.raises(ValueError):                          # nothing resident
            ctx.speed_spectrum(np.zeros(1), np.zeros(1, dtype=bool), atoms=[0])


# ---- 5. bands -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [(0, np.inf), (0.05, 0.3), (0.0995, 0.1005)], ids=["default", "0.05-0.3", "one_bin"])
def test_bands(band):
    from sitator_amd import AverageVibrationalFrequency
    traj = V.random_walk(1001, 5, seed=31)
    mask = np.array([True, False, True, True, False])
    ref = V.restatement(traj, mask, *band)
    if band[0] > 0.09:
        assert ref["fmask"].sum() == 1                           # rfftfreq(1000)[100] alone
    with Context() as ctx:
        check_against_numpy(ref, *host_call(ctx, traj, mask, band))
    got = AverageVibrationalFrequency(*band).compute_avg_vibrational_freq(traj, mask, return_stdev=True)
    check_over_atoms(got, ref["mean"], ref["std"])


def test_empty_band_is_the_reference_assertion():
    from sitator_amd import AverageVibrationalFrequency
    traj = V.random_walk(101, 2, seed=32)
    with pytest.raises(AssertionError, match="Trajectory too short"):
        AverageVibrationalFrequency(0.101, 0.109).compute_avg_vibrational_freq(traj, [0, 1])
    with pytest.raises(AssertionError, match="Trajectory too short"):
        AverageVibrationalFrequency(0.6, 0.9).compute_avg_vibrational_freq(traj, [0, 1])


# ---- 6. the operator ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", VG.names)
def test_operator_matches_the_reference(name):
    from sitator_amd import AverageVibrationalFrequency
    traj, mask, kw, expected = VG.case(name)
    keep = traj.copy()
    op = AverageVibrationalFrequency(min_frequency=kw["min_frequency"], max_frequency=kw["max_frequency"])
    got = op.compute_avg_vibrational_freq(traj, mask, return_stdev=kw["return_stdev"])
    assert isinstance(got, tuple) == kw["return_stdev"]
    check_over_atoms(got, *expected)
    assert np.array_equal(traj, keep)


def test_operator_masks_and_stdev():
    from sitator_amd import AverageVibrationalFrequency
    traj = V.random_walk(301, 6, seed=41)
    op = AverageVibrationalFrequency()
    mask = np.array([True, False, False, True, True, False])
    a = op.compute_avg_vibrational_freq(traj, mask, return_stdev=True)
    b = op.compute_avg_vibrational_freq(traj, np.where(mask)[0], return_stdev=True)
    assert a == b and isinstance(a, tuple) and len(a) == 2
    assert op.compute_avg_vibrational_freq(traj, mask) == a[0]
    ref = V.restatement(traj, mask)
    check_over_atoms(a, ref["mean"], ref["std"])


def test_operator_errors():
    from sitator_amd import AverageVibrationalFrequency
    traj = V.random_walk(50, 3, seed=42)
    op = AverageVibrationalFrequency()
    with pytest.raises(AssertionError, match="Trajectory too short"):
        op.compute_avg_vibrational_freq(traj[:2], [0, 1])                                # F == 2: the band is empty
    with pytest.raises(ValueError):
        op.compute_avg_vibrational_freq(traj[:1], [0, 1])                                # F == 1
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'double' but got 'float32'"):
        op.compute_avg_vibrational_freq(traj.astype(np.float32), [0, 1])
    still = traj.copy()
    still[:, 1] = still[0, 1]
    with pytest.raises(ZeroDivisionError):
        op.compute_avg_vibrational_freq(still, [0, 1, 2])                                # atom 1 never moves
    assert np.isfinite(op.compute_avg_vibrational_freq(still, [0, 2]))
    with pytest.raises(AssertionError):
        AverageVibrationalFrequency(min_frequency=-0.1)


def test_operator_on_the_frames_an_analysis_left_resident():
    from sitator_amd import AverageVibrationalFrequency, LandmarkAnalysis, SiteNetwork, Structure
    c = G.Case("c1_hex_scgrid")
    sn = SiteNetwork(Structure(c.ref_positions, c.cell), c.static_mask, c.mobile_mask)
    sn.centers = c.centers
    sn.vertices = c.vertices
    frames = np.ascontiguousarray(c.frames)
    la = LandmarkAnalysis(verbose=False, **c.kwargs("dotprod"))
    op = AverageVibrationalFrequency(0.01, 0.45)
    with pytest.raises(ValueError):
        op.compute_for_analysis(la)                                                      # has not run
    st = la.run(sn, frames)
    version = la._ctx.labels_version
    exp = op.compute_avg_vibrational_freq(frames, c.mobile_mask, return_stdev=True)
    assert op.compute_for_analysis(la, return_stdev=True) == exp                         # bit-equal
    assert op.compute_for_analysis(la, mask=c.mobile_mask, return_stdev=True) == exp
    assert op.compute_for_analysis(la, mask=np.where(c.mobile_mask)[0]) == exp[0]
    static = op.compute_for_analysis(la, mask=c.static_mask)
    assert static == op.compute_avg_vibrational_freq(frames, c.static_mask)
    with pytest.raises(IndexError):
        op.compute_for_analysis(la, mask=[frames.shape[1]])
    assert la._ctx.labels_version == version
    assert np.array_equal(st.traj, c.out("dotprod")["labels"])
    assert np.array_equal(resident_frames(la._ctx), frames)


def test_operator_refuses_frames_recentred_on_the_device():
    from sitator_amd import AverageVibrationalFrequency, LandmarkAnalysis, RecenterTrajectory, SiteNetwork, Structure, synth
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
    with pytest.raises(ValueError, match="recent"):
        AverageVibrationalFrequency().compute_for_analysis(la)


def test_operator_refuses_frame_shards():
    from sitator_amd import AverageVibrationalFrequency, LandmarkAnalysis, SiteNetwork, Structure
    c = G.Case("c1_hex_scgrid")
    sn = SiteNetwork(Structure(c.ref_positions, c.cell), c.static_mask, c.mobile_mask)
    sn.centers = c.centers
    sn.vertices = c.vertices
    la = LandmarkAnalysis(verbose=False, devices=[0, 0], **c.kwargs("dotprod"))
    la.run(sn, np.ascontiguousarray(c.frames))
    with pytest.raises(NotImplementedError):
        AverageVibrationalFrequency().compute_for_analysis(la)
