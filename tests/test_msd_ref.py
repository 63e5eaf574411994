"""CPU-only: the numpy restatement of the mean squared displacement (tests/msd_ref.py) against closed forms, so that what the
device is compared with is itself pinned: a straight line, a sinusoid, a ballistic path wrapped through a triclinic cell
(known integer images), the all-lag emulation against the long-double sums, and ``diffusion_coefficient`` on a line."""
import numpy as np
import pytest

from tests import msd_ref as R


def test_cells_are_as_tall_as_the_inputs_need():
    for cell in R.CELLS.values():
        assert np.all(R.heights(cell) >= 3.0)


def test_straight_line():
    """x = v t: msd(tau) = v_a^2 tau^2 per axis, r4 = |v|^4 tau^4."""
    F, v = 40, np.array([0.25, -0.5, 0.125])                       # dyadic: every product below is exact
    x = (np.arange(F)[:, None, None] * v[None, None, :]).astype(np.float64)
    y = R.series(x)
    lags = np.arange(F)
    msd, r4 = R.msd_direct(y, lags)
    assert np.array_equal(msd[0].astype(np.float64), (v * v)[:, None] * (lags * lags)[None, :])
    assert np.array_equal(r4[0].astype(np.float64), np.sum(v * v) ** 2 * lags.astype(np.float64) ** 4)
    for a in range(3):
        emu = R.msd_fft_emulation(y[0, a], F)
        assert np.max(np.abs(emu - np.asarray(msd[0, a], dtype=np.float64)) * (F - lags)) <= 1e-13 * float(R.sum_squares(y)[0, a])


def test_sinusoid():
    """x = sin(w t) over whole periods: (1/(F-tau)) sum (x[t+tau]-x[t])^2 = 2 sin^2(w tau / 2) (1 + mean cos(w (2 t + tau))),
    and the cosine's sum has a closed form."""
    F, periods = 600, 6
    w = 2.0 * np.pi * periods / F
    t = np.arange(F)
    x = np.zeros((F, 1, 3))
    x[:, 0, 0] = np.sin(w * t)
    y = R.series(x)
    lags = np.array([1, 7, 50, 100, 299, 300, 599])
    msd, _ = R.msd_direct(y, lags)
    for l, tau in enumerate(lags):
        n = F - tau
        # sum_{t<n} cos(w (2 t + tau)) = sin(n w) cos(w (n - 1) + w tau) / sin(w)
        csum = np.sin(n * w) * np.cos(w * (n - 1) + w * tau) / np.sin(w)
        expect = 2.0 * np.sin(w * tau / 2.0) ** 2 * (1.0 + csum / n)
        assert abs(float(msd[0, 0, l]) - expect) <= 1e-12
    assert np.all(msd[0, 1:] == 0)


def test_ballistic_path_through_a_triclinic_cell():
    """A straight path wrapped into the cell: the images are the floors of its fractional coordinates, the unwrapped
    series the path itself, max_residual the fractional step."""
    F = 400
    v = np.array([0.11, -0.07, 0.05])
    x = np.array([0.3, 0.4, 0.2]) + np.arange(F)[:, None] * v[None, :]
    x = x[:, None, :]
    wrapped, fl = R.wrap_into(x, R.TRICLINIC)
    assert np.abs(fl).max() >= 2                                     # the path leaves the cell more than once
    xu, images, res = R.unwrap(wrapped, R.TRICLINIC)
    assert np.array_equal(images[0], fl[:, 0] - fl[0, 0])
    np.testing.assert_allclose(xu - xu[0], x - x[0], rtol=0, atol=1e-12)
    fstep = np.abs(v @ np.linalg.inv(R.TRICLINIC))
    assert abs(res - fstep.max()) < 1e-12 and res < 0.25
    # an unwrapped path passes through bit for bit
    xu2, images2, _ = R.unwrap(x, R.TRICLINIC)
    assert np.array_equal(xu2, x) and not images2.any()
    msd, _ = R.msd_direct(R.series(wrapped, R.TRICLINIC), [0, 1, 10])
    np.testing.assert_allclose(msd[0].astype(np.float64), (v * v)[:, None] * np.array([0.0, 1.0, 100.0])[None, :], rtol=1e-9)


def test_image_rounding():
    ulp = 2.0 ** -53
    f = np.array([0.5, -0.5, 0.5 + ulp, 0.5 - ulp / 2, 1.5, -1.5, 2.5, np.nan, np.inf, -np.inf, 2.0 ** 30, 2.0 ** 30 - 1.0, -0.0])
    n, res = R.image(f)
    assert list(n) == [0, 0, 1, 0, 2, -2, 2, 0, 0, 0, 0, 2 ** 30 - 1, 0]
    assert list(res[:3]) == [0.5, 0.5, 0.5 - ulp] and list(res[7:11]) == [-1.0] * 4


@pytest.mark.parametrize("F", [1, 2, 1023, 1024, 1025, 2049, 3000])
def test_prefix_order_is_a_prefix_sum(F):
    y = np.random.default_rng(F).normal(size=F)
    P = R.prefix_squares(y)
    exact = np.concatenate([[0.0], np.cumsum((y.astype(np.longdouble)) ** 2)])
    assert P[0] == 0.0 and len(P) == F + 1
    assert np.max(np.abs(P - exact)) <= 16 * np.finfo(np.float64).eps * float(exact[-1])
    assert R.n_chunks(F) == -(-F // 1024)


@pytest.mark.parametrize("F,drift", [(2, None), (3, None), (5, None), (33, None), (513, None), (1000, (0.01, 0.0, -0.02)), (4099, None)])
def test_emulation_against_the_sums(F, drift):
    """The all-lag algorithm in numpy stays far inside the bound the device is held to (1e-13 in units of sum y^2 / (F - tau));
    what it gives here is recorded in tests/test_gpu_msd.py."""
    y = R.series(R.random_walk(F, 1, seed=F, drift=drift))
    lags = np.arange(F)
    ref, _ = R.msd_direct(y, lags)
    for a in range(3):
        emu = R.msd_fft_emulation(y[0, a], F)
        err = np.max(np.abs(emu - np.asarray(ref[0, a], dtype=np.float64)) * (F - lags)) / float(R.sum_squares(y)[0, a])
        assert err <= 1e-14


def test_plan_arithmetic():
    assert R.padded_length(2) == 4 and R.padded_length(512) == 1024 and R.padded_length(513) == 2048
    assert R.atom_bytes(257, 129, False) == 3 * (2304 + 1280 + 2304 + 256 + 1024 * 16 + 1280)
    assert R.batch(257, 5, 129, False, False, R.atom_bytes(257, 129, False)) == (1, 5)
    assert R.batch(257, 5, 129, False, False, R.atom_bytes(257, 129, False) - 1) is None
    assert R.batch(257, 5, 129, False, True, R.atom_bytes(257, 129, False)) is None
    assert R.batch(257, 5, 3, True, True, R.fixed_bytes(257, True) + 2 * R.atom_bytes(257, 3, True) + 100) == (2, 3)


def test_diffusion_coefficient_on_a_line():
    from sitator_amd.dynamics import diffusion_coefficient
    D, c = 0.0375, 0.21
    lags = np.arange(1, 400)
    for dt, dims in [(1.0, 3), (0.002, 3), (2.0, 1)]:
        msd = 2 * dims * D * (lags * dt) + c
        got, icpt = diffusion_coefficient(lags, msd, timestep=dt, dimensions=dims)
        np.testing.assert_allclose(got, D, rtol=1e-12)
        np.testing.assert_allclose(icpt, c, rtol=1e-10)
    got, _ = diffusion_coefficient(lags, np.where(lags < 100, 0.0, 6 * D * lags + c), fit_range=(100, 399))
    np.testing.assert_allclose(got, D, rtol=1e-12)
    with pytest.raises(ValueError):
        diffusion_coefficient(lags[:1], lags[:1])
