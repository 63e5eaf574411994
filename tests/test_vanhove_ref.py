"""CPU-only: the numpy restatement of the van Hove correlation function (tests/vanhove_ref.py) held to brute force and to
closed forms, so that the GPU tests compare the kernels with something that is itself pinned."""
import numpy as np

from tests import msd_ref as R
from tests import vanhove_ref as V


def test_minimum_image_against_a_brute_force_over_729_images():
    """A triclinic cell, r_max at the limit: the rounded fractional difference finds the same pairs within r_max as the
    shortest of 9^3 images does, at the same distances (to rounding: the brute force adds the lattice vector in Cartesian
    coordinates)."""
    cell = R.TRICLINIC
    cm, ci = V.cell_matrices(cell)
    r_max = 0.5 * V.hmin(cell) * V.MARGIN
    assert V.rmax_ok(r_max, V.hmin(cell)) and not V.rmax_ok(np.nextafter(r_max, 10.0), V.hmin(cell))
    np.testing.assert_allclose(V.hmin(cell), R.heights(cell).min(), rtol=1e-14)
    rng = np.random.default_rng(1)
    pa, pb = rng.uniform(-6.0, 6.0, size=(4000, 3)), rng.uniform(-6.0, 6.0, size=(4000, 3))
    r2 = V.image_r2(V.fractional(pb, ci) - V.fractional(pa, ci), cm)
    n = np.arange(-4, 5)
    shifts = np.stack(np.meshgrid(n, n, n, indexing="ij"), axis=-1).reshape(-1, 3) @ cell
    brute = np.min(np.sum(((pb - pa)[:, None, :] + shifts[None, :, :]) ** 2, axis=2), axis=1)
    inside, inside_brute = r2 < r_max * r_max, brute < r_max * r_max
    assert np.array_equal(inside, inside_brute) and 500 < inside.sum() < 3500
    np.testing.assert_allclose(r2[inside], brute[inside], rtol=1e-12)
    # and the bins they fall into: the same but for a distance within rounding of an edge
    e2 = V.edges2(r_max, 64)
    assert np.count_nonzero(V.bin_of(r2, e2) != V.bin_of(brute, e2)) <= 2


def test_simple_cubic_lattice_at_rest_has_its_shell_populations():
    """27 atoms on a 3 x 3 x 3 simple cubic lattice of spacing 2 in a cell of edge 6: 6 neighbours at 2, 12 at 2 sqrt 2,
    8 at 2 sqrt 3 (r_max is just below 3, half the cell)."""
    g = np.arange(3) * 2.0
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    x = np.repeat(pos[None], 4, axis=0) + 0.37                   # at rest, off the origin
    cell = np.eye(3) * 6.0
    r_max, n_bins = 2.999, 2999                                   # bins of 0.001
    idx = np.arange(27)
    counts = V.distinct(x, cell, idx, idx, True, [0, 2], 1, r_max, n_bins)
    for row, origins in zip(counts, (4, 2)):
        per = {}
        for k in np.nonzero(row[:n_bins])[0]:
            per[round(k * 0.001, 1)] = per.get(round(k * 0.001, 1), 0) + int(row[k])
        # the 26 other atoms: 6 + 12 + 8 within r_max, none beyond (sqrt 12 = 3.46 is the image of a nearer one)
        assert {k: v // (27 * origins) for k, v in per.items()} == {2.0: 6, 2.8: 12}
        assert int(row[n_bins]) == 27 * origins * 8 and int(row.sum()) == origins * 27 * 26
    # with r_max beyond sqrt 12 the third shell would be in; in this cell it cannot be: 2 sqrt 3 > 3.  A 4^3 lattice shows it
    g = np.arange(4) * 2.0
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    idx = np.arange(64)
    # (bins of 0.3: the shells at 2, 2.83 and 3.46 lie inside bins 6, 9 and 11, away from their edges)
    row = V.distinct(pos[None] + 0.11, np.eye(3) * 8.0, idx, idx, True, [0], 1, 3.9, 13)[0]
    assert [int(v) for v in row[:13]] == [0, 0, 0, 0, 0, 0, 64 * 6, 0, 0, 64 * 12, 0, 64 * 8, 0] and int(row.sum()) == 64 * 63
    # the second selection as a list of its own: a pair of an atom with itself is a pair like any other, at distance 0
    row_ab = V.distinct(pos[None] + 0.11, np.eye(3) * 8.0, idx, idx, False, [0], 1, 3.9, 13)[0]
    assert int(row_ab[0]) == 64 and np.array_equal(row_ab[1:], row[1:])


def test_self_part_of_uniform_motion_falls_in_one_bin():
    """x = v t, |v| = 0.073: every displacement at lag tau is 0.073 tau, whatever the origin - 1.46 tau bins of 0.05, never
    near an edge at these lags; beyond r_max it is overflow.  No unwrapping is involved (the cell is far larger than the path)."""
    F, v = 50, np.array([0.02, -0.03, 0.06]) * (0.073 / np.sqrt(0.02 ** 2 + 0.03 ** 2 + 0.06 ** 2))
    x = (np.arange(F)[:, None, None] * v[None, None, :]) + np.array([[1.0, 2.0, 3.0], [4.0, 4.0, 4.0]])[None]
    cell = np.eye(3) * 40.0
    r_max, n_bins = 2.0, 40                                        # bins of 0.05
    lags = [0, 1, 5, 10, 27, 28, 49]
    for unwrap in (True, False):
        counts, res = V.self_part(x, cell, [0, 1], lags, 1, r_max, n_bins, unwrap=unwrap)
        assert res < 0.01
        for row, tau in zip(counts, lags):
            k = int(np.floor(0.073 * tau / 0.05))
            origins = V.n_origins(F, tau, 1)
            assert origins == F - tau and int(row.sum()) == 2 * origins
            assert int(row[min(k, n_bins)]) == 2 * origins, (tau, k, np.nonzero(row)[0])
    counts3, _ = V.self_part(x, cell, [0, 1], lags, 3, r_max, n_bins)
    assert [int(r.sum()) for r in counts3] == [2 * ((F - 1 - tau) // 3 + 1) for tau in lags]


def test_ideal_gas_normalises_to_one():
    """Uniform random positions, redrawn in every frame: g(r) and G_d / rho are 1 within the counting noise, the self density
    integrates to one minus the overflow share."""
    from sitator_amd.dynamics import VanHoveResult, _vanhove_edges
    cell = R.TRICLINIC
    rng = np.random.default_rng(5)
    F, n = 40, 60
    x = rng.random((F, n, 3)) @ cell
    r_max, n_bins = 0.5 * V.hmin(cell) * V.MARGIN, 8
    lags = np.array([0, 3])
    a, b = np.arange(0, 25), np.arange(25, 60)
    dc = V.distinct(x, cell, a, b, False, lags, 1, r_max, n_bins)
    sc, _ = V.self_part(x, cell, a, lags, 1, r_max, n_bins, unwrap=False)
    origins = np.array([V.n_origins(F, t, 1) for t in lags])
    res = VanHoveResult(lags, _vanhove_edges(r_max, n_bins), origins, len(a), len(a) * len(b), abs(np.linalg.det(cell)), sc, dc, 0.0)
    expected = origins[:, None] * len(a) * len(b) * (4 * np.pi / 3) * (res.edges[1:] ** 3 - res.edges[:-1] ** 3) / abs(np.linalg.det(cell))
    assert expected[:, 2:].min() > 100                            # enough pairs per bin for five standard deviations to mean something
    assert np.all(np.abs(res.distinct - 1.0)[:, 2:] < 5.0 / np.sqrt(expected[:, 2:]))
    assert np.array_equal(res.edges * res.edges, V.edges2(r_max, n_bins))
    dr = r_max / n_bins
    share = sc[:, n_bins] / (origins * len(a))
    np.testing.assert_allclose(res.self_density.sum(axis=1) * dr, 1.0 - share, rtol=1e-12)
    assert np.array_equal(sc[0, :n_bins], [len(a) * F] + [0] * (n_bins - 1))       # lag 0: every displacement is 0
    same = VanHoveResult(lags, res.edges, origins, len(a), len(a) * (len(a) - 1), abs(np.linalg.det(cell)), None,
                         V.distinct(x, cell, a, a, True, lags, 1, r_max, n_bins), 0.0)
    assert same.self_density is None and np.all(same.distinct_counts.sum(axis=1) == origins * len(a) * (len(a) - 1))
