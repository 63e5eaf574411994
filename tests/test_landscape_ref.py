"""CPU-only: the restatement tests/landscape_ref.py pinned - against ``barrier_ref.mobile_energy`` (``math.fsum``, correctly rounded)
at every voxel of small grids, on an atom, on a value computed by hand, and on the designed tetragonal host.

The bound.  A float64 sum of ``n`` terms taken one after the other errs by at most about ``n * 2^-53 * sum |phi|`` against the
correctly rounded sum (the bound tests/test_gpu_barrier.py derives); ``n`` is asserted."""
import numpy as np
import pytest

from tests import barrier_ref as BR
from tests import landscape_ref as LR


def lattice(cell, S, seed):
    rng = np.random.default_rng(seed)
    pos = rng.random((S, 3)) @ cell + (rng.integers(-1, 2, size=(S, 3)) @ cell if seed % 2 else 0.0)
    return pos, 0.5 + rng.random(S), 0.8 + 0.4 * rng.random(S)


@pytest.mark.parametrize("name, grid, S, rc_heights", [("CUBIC", (2, 3, 5), 5, 0.4), ("TRICLINIC", (3, 2, 4), 7, 0.4),
                                                       ("SMALL_TRICLINIC", (2, 3, 5), 2, 2.2), ("SMALL_TRICLINIC", (1, 1, 1), 5, 0.9)])
def test_flat_sum_against_fsum_at_every_voxel(name, grid, S, rc_heights):
    cell = getattr(BR, name)
    rc = rc_heights * BR.heights(cell).min()
    pos, eps, sigma = lattice(cell, S, 11 + S)
    most = 0
    for v in range(grid[0] * grid[1] * grid[2]):
        x = LR.center(cell, grid, LR.unflatten(grid, v))
        e, n = LR.energy(cell, pos, eps, sigma, rc, x)
        want, abs_sum, n_want = BR.mobile_energy(cell, pos, eps, sigma, rc, x)
        assert n == n_want and n <= 2000
        assert abs(e - want) <= n * 2.0 ** -53 * abs_sum, (v, e, want)
        most = max(most, n)
    assert most > (50 if rc_heights > 1 else 0)


def test_terms_are_sorted_and_the_reach_is_generous():
    cell = BR.SMALL_TRICLINIC
    rc = 2.2 * BR.heights(cell).min()
    pos, eps, sigma = lattice(cell, 3, 5)
    x = LR.center(cell, (2, 3, 5), (1, 2, 3))
    p, dd, atom, m = LR.voxel_terms(cell, pos, eps, sigma, rc, x)
    keys = [(int(a),) + tuple(int(v) for v in t) for a, t in zip(atom, m)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and len(keys) > 100
    wider = LR.voxel_terms(cell, pos, eps, sigma, rc, x, extra=3)
    assert wider[0].tobytes() == p.tobytes() and np.array_equal(wider[3], m)


def test_a_voxel_centre_on_an_atom_is_plus_infinity():
    for cell in (BR.CUBIC, BR.TRICLINIC, BR.SMALL_TRICLINIC):
        grid = (3, 5, 7)
        on = LR.center(cell, grid, (1, 4, 2))                       # the voxel-centre arithmetic itself
        pos = np.array([on, on + 0.37 * cell[0] + 0.2 * cell[2]])
        e, n = LR.energy(cell, pos, [1.0, 0.7], [1.0, 1.2], 0.45 * BR.heights(cell).min(), on)
        assert e == np.inf and n >= 1
        near, _ = LR.energy(cell, pos, [1.0, 0.7], [1.0, 1.2], 0.45 * BR.heights(cell).min(), LR.center(cell, grid, (1, 3, 2)))
        assert np.isfinite(near)
        all_e = LR.energies(cell, pos, [1.0, 0.7], [1.0, 1.2], 0.45 * BR.heights(cell).min(), grid)
        assert np.isinf(all_e).sum() == 1 and all_e[(1 * 5 + 4) * 7 + 2] == np.inf and not np.isnan(all_e).any()


def test_a_single_atom_by_hand():
    """One atom at the origin of a 10 A cube, rc = 3, sigma = 1, eps = 1; voxel (0, 0, 0) of the grid (5, 5, 5) has its centre at
    (1, 1, 1): dd = 3, s6 = 1 / 27, phi = 4 / 27 (1 / 27 - 1) - e0, e0 = 4 / 729 (1 / 729 - 1)."""
    cell = np.eye(3) * 10.0
    x = LR.center(cell, (5, 5, 5), (0, 0, 0))
    assert x.tolist() == [1.0, 1.0, 1.0]
    e, n = LR.energy(cell, np.zeros((1, 3)), [1.0], [1.0], 3.0, x)
    q, q0 = 1.0 / 3.0, 1.0 / 9.0
    s6, s60 = (q * q) * q, (q0 * q0) * q0
    assert n == 1 and e == (4.0 * s6) * (s6 - 1.0) - (4.0 * s60) * (s60 - 1.0)
    assert abs(e - (4.0 / 27.0 * (1.0 / 27.0 - 1.0) - 4.0 / 729.0 * (1.0 / 729.0 - 1.0))) < 1e-15
    # the voxel across the corner sees the atom's image (-1, -1, -1) at the same distance
    far = LR.voxel_terms(cell, np.zeros((1, 3)), [1.0], [1.0], 3.0, LR.center(cell, (5, 5, 5), (4, 4, 4)))
    assert far[3].tolist() == [[1, 1, 1]] and far[0][0] == e


def test_the_designed_host_has_its_minima_saddles_and_order():
    cell, pos, numbers, grid = LR.tetragonal_host()
    E = LR.energies(cell, pos, np.full(8, LR.TET_EPS), np.full(8, LR.TET_SIGMA), LR.TET_RC, grid)
    body, wide, narrow = LR.tetragonal_voxels()
    atoms = np.nonzero(np.isinf(E))[0]
    assert len(atoms) == 8 and len(set(body) | set(wide) | set(narrow)) == 32
    # by symmetry every voxel of a kind has the same terms, in another order: equal to a few ulps
    for kind in (body, wide, narrow):
        assert np.ptp(E[kind]) <= 1e-13 * np.abs(E[kind]).max()
    assert E[body].max() < E[wide].min() <= E[wide].max() < E[narrow].min()
    assert E.min() == E[body].min() and set(np.argsort(E, kind="stable")[:8]) == set(body)
