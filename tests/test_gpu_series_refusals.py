"""What the frame-series entry points (sit_msd, sit_vanhove, sit_scattering, sit_density) say when they refuse a call: the
exception and the whole message, written out here and not taken from the library, for an atom, a lag, a cell, the resident
frames - and, where an input is wrong in two ways, which of the two is reported."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F, A = 4, 3
CELL = np.eye(3) * 12.0
FLAT = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]])        # determinant 0, exactly, in integers


def host_frames():
    return np.random.default_rng(7).uniform(0.0, 12.0, (F, A, 3))


@pytest.fixture(scope="module")
def lib():
    from sitator_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible")
    return _lib


@pytest.fixture(scope="module")
def resident(lib):
    with lib.HipContext(CELL) as ctx:
        ctx.set_basis(np.full((1, 3), 6.0), np.zeros((1, 1), dtype=np.int64), np.ones((1, 1)), 1.5, 30, 1.0)   # one static atom, one site
        ctx.set_frames(host_frames(), np.arange(1), np.arange(1, A))
        yield ctx


@pytest.fixture(scope="module")
def empty(lib):
    with lib.HipContext(CELL) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def singular(lib):
    # A context takes its cell when it is made and has no other setter.  HipContext.__init__ inverts the cell with
    # np.linalg.inv before it calls sit_create; that is the one thing of its inside this fixture leans on.  The inverse is made
    # up: a singular cell has none, and whether numpy's LU meets an exact zero pivot is its own affair.
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(np.linalg, "inv", lambda m: np.eye(3))
        ctx = lib.HipContext(FLAT)
    with ctx:
        yield ctx


def msd(ctx, positions=None, atoms=(1, 2), **kw):
    return ctx.msd(positions=positions, atoms=None if positions is not None else list(atoms), **kw)


def vanhove(ctx, positions=None, a=(1,), b=(2,), lags=(0, 1)):
    from sitator_amd import _lib_vanhove
    return _lib_vanhove.vanhove(ctx, list(a), list(b), list(lags), 1.0, 4, positions=positions)


def scattering(ctx, positions=None, a=(1,), b=(2,), lags=(0, 1)):
    from sitator_amd import _lib_scattering
    return _lib_scattering.scattering(ctx, list(a), list(b), [[1, 0, 0]], list(lags), positions=positions)


def density(ctx, positions=None, atoms=(1, 2)):
    from sitator_amd import _lib_density
    return _lib_density.density(ctx, list(atoms), (2, 2, 2), positions=positions)


def refused(text, call, *args, **kw):
    with pytest.raises(ValueError) as info:
        call(*args, **kw)
    assert str(info.value) == text


class Sizes(object):
    """The context says it holds F frames of A atoms for the length of the block.  It leans on HipContext keeping the sizes of
    the resident frames as the plain attributes ``F`` and ``A`` that ``_frames`` / ``_selection`` hand to the library (as
    test_gpu_msd.py and test_gpu_vanhove.py do with ``ctx.F += 1``)."""

    def __init__(self, ctx, F, A):
        self.ctx, self.sizes = ctx, (F, A)

    def __enter__(self):
        self.kept = (self.ctx.F, self.ctx.A)
        self.ctx.F, self.ctx.A = self.sizes

    def __exit__(self, *exc):
        self.ctx.F, self.ctx.A = self.kept


def test_the_calls_are_taken_as_they_stand(resident):
    assert msd(resident)[0].shape == (2, 3, 3) and msd(resident, positions=host_frames())[0].shape == (A, 3, 3)
    assert vanhove(resident)[1].shape == (2, 5) and vanhove(resident, positions=host_frames())[1].shape == (2, 5)
    assert scattering(resident)[1].shape == (2, 1) and scattering(resident, positions=host_frames())[1].shape == (2, 1)
    assert density(resident)[0].sum() == 2 * F and density(resident, positions=host_frames())[0].sum() == 2 * F


def test_an_atom_beyond_the_frame(resident):
    x = host_frames()
    refused("sit_msd: atom 3 is outside the 3 atoms of a frame", msd, resident, atoms=[1, A])
    refused("sit_msd: atom -1 is outside the 3 atoms of a frame", msd, resident, atoms=[-1, 1])
    for pos in (None, x):
        refused("sit_vanhove: atom 3 is outside the 3 atoms of a frame", vanhove, resident, pos, a=[1, A])
        refused("sit_vanhove: atom -1 is outside the 3 atoms of a frame", vanhove, resident, pos, b=[-1])
        refused("sit_vanhove: atom 3 is outside the 3 atoms of a frame", vanhove, resident, pos, a=[A], b=[-1])       # a before b
        refused("sit_scattering: atom 3 is outside the 3 atoms of a frame", scattering, resident, pos, b=[0, A])
        refused("sit_scattering: atom -1 is outside the 3 atoms of a frame", scattering, resident, pos, a=[-1])
        refused("sit_scattering: atom 3 is outside the 3 atoms of a frame", scattering, resident, pos, a=[A], b=[-1])
        refused("sit_density: atom 3 is outside [0, 3)", density, resident, pos, atoms=[1, A])
        refused("sit_density: atom -1 is outside [0, 3)", density, resident, pos, atoms=[-1])


def test_a_lag_beyond_the_frames(resident):
    x = host_frames()
    for pos in (None, x):
        refused("sit_msd: lag 4 is outside [0, 3]", msd, resident, pos, lags=[0, F])
        refused("sit_msd: lag -1 is outside [0, 3]", msd, resident, pos, lags=[-1])
        refused("sit_vanhove: lag 4 is outside [0, 3]", vanhove, resident, pos, lags=[0, F])
        refused("sit_vanhove: lag -1 is outside [0, 3]", vanhove, resident, pos, lags=[-1, F])
        refused("sit_scattering: lag 4 is outside [0, 3]", scattering, resident, pos, lags=[F, -1])
        refused("sit_scattering: lag -1 is outside [0, 3]", scattering, resident, pos, lags=[3, -1])
    assert msd(resident, lags=[F - 1])[0].shape == (2, 3, 1) and vanhove(resident, lags=[F - 1])[1].shape == (1, 5)


def test_a_singular_cell(singular):
    x = host_frames()
    refused("sit_msd: a degenerate cell cannot unwrap a trajectory", msd, singular, x)
    refused("sit_msd: a degenerate cell cannot unwrap a trajectory", msd, singular, x, lags=[1])
    assert msd(singular, x, unwrap=False)[0].shape == (A, 3, 3)               # no unwrapping: the cell is not looked at
    refused("sit_vanhove: a degenerate cell", vanhove, singular, x)
    refused("sit_scattering: a degenerate cell", scattering, singular, x)
    refused("sit_density: a degenerate cell", density, singular, x)


def test_nothing_resident(empty):
    # a context without frames says it holds none of them: the sizes are refused before anybody asks where the frames are
    refused("sit_msd: at least two frames needed", msd, empty)
    refused("sit_vanhove: 1 to 2^29 frames are needed", vanhove, empty)
    refused("sit_scattering: 1 to 2^29 frames are needed", scattering, empty)
    refused("sit_density: 1 to 2^29 frames are needed", density, empty)
    with Sizes(empty, F, A):
        refused("sit_msd: no resident frames (sit_set_frames first)", msd, empty)
        refused("sit_vanhove: no resident frames (sit_set_frames first)", vanhove, empty)
        refused("sit_scattering: no resident frames (sit_set_frames first)", scattering, empty)
        refused("sit_density: no resident frames (sit_set_frames first)", density, empty)


def test_sizes_other_than_the_resident_ones(resident):
    with Sizes(resident, F + 1, A):
        refused("sit_msd: F is not the number of resident frames", msd, resident)
        refused("sit_vanhove: F or A is not that of the resident frames", vanhove, resident)
        refused("sit_scattering: F or A is not that of the resident frames", scattering, resident)
        refused("sit_density: F or A is not that of the resident frames", density, resident)
    with Sizes(resident, F, A + 1):
        refused("sit_vanhove: F or A is not that of the resident frames", vanhove, resident)
        refused("sit_scattering: F or A is not that of the resident frames", scattering, resident)
        refused("sit_density: F or A is not that of the resident frames", density, resident)
    assert density(resident)[0].sum() == 2 * F                                # and the context still works


def test_which_of_two_faults_is_reported(resident, singular, empty):
    x = host_frames()
    # a bad lag together with a bad atom: the lag
    refused("sit_msd: lag 4 is outside [0, 3]", msd, resident, atoms=[A], lags=[F])
    for pos in (None, x):
        refused("sit_vanhove: lag -1 is outside [0, 3]", vanhove, resident, pos, a=[A], lags=[-1])
        refused("sit_scattering: lag 4 is outside [0, 3]", scattering, resident, pos, b=[-1], lags=[F])
    # a bad lag under a singular cell: the lag; a bad atom under it: the cell
    refused("sit_msd: lag 4 is outside [0, 3]", msd, singular, x, lags=[F])
    refused("sit_vanhove: lag 4 is outside [0, 3]", vanhove, singular, x, lags=[F])
    refused("sit_scattering: lag 4 is outside [0, 3]", scattering, singular, x, lags=[F])
    refused("sit_vanhove: a degenerate cell", vanhove, singular, x, a=[A])
    refused("sit_scattering: a degenerate cell", scattering, singular, x, a=[A])
    refused("sit_density: a degenerate cell", density, singular, x, atoms=[A])
    # a bad atom where nothing is resident: the frames
    with Sizes(empty, F, A):
        refused("sit_msd: no resident frames (sit_set_frames first)", msd, empty, atoms=[A])
        refused("sit_vanhove: no resident frames (sit_set_frames first)", vanhove, empty, a=[A])
        refused("sit_scattering: no resident frames (sit_set_frames first)", scattering, empty, a=[-1])
        refused("sit_density: no resident frames (sit_set_frames first)", density, empty, atoms=[A])
        refused("sit_vanhove: lag 4 is outside [0, 3]", vanhove, empty, lags=[F])                    # and a bad lag before them
