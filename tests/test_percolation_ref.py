"""CPU-only: the restatement of DensityPercolation (tests/percolation_ref.py) held to designed answers - sets whose components, loop
lattices and levels can be read off.  Everything is an integer or the bytes of a double: no tolerance."""
import numpy as np
import pytest

from tests import percolation_ref as R

DESIGNED = R.designed()


def summary(grid, level, connectivity):
    labels, roots, sizes, rank, basis = R.components(grid, level, connectivity)
    return labels, roots, [(int(s), int(r), b.tolist()) for s, r, b in zip(sizes, rank, basis)]


@pytest.mark.parametrize("case", DESIGNED, ids=[c[0] for c in DESIGNED])
def test_designed_components(case):
    name, grid, level, connectivity, expected = case
    labels, roots, got = summary(grid, level, connectivity)
    assert got == expected
    flat = labels.reshape(-1)
    assert np.array_equal(flat >= 0, grid.reshape(-1) >= level) and np.all(np.diff(roots) > 0)
    assert np.array_equal(np.unique(flat[flat >= 0]), roots) and np.all(flat[roots] == roots)          # a root is its own label
    assert np.all(flat[flat >= 0] <= np.flatnonzero(flat >= 0))                                        # ... and the lowest index


def test_the_double_loop_is_not_primitive_and_needs_three_dimensions():
    (case,) = [c for c in DESIGNED if c[0] == "double_loop_2_0_0"]
    _, roots, got = summary(case[1], 1.0, 26)
    assert len(roots) == 1 and got[0][2][0] == [2, 0, 0]            # twice round the cell before it closes: (1, 0, 0) is no loop
    assert R.hnf([(2, 0, 0)])[0][0] == [2, 0, 0] and R.hnf([(2, 0, 0), (1, 0, 0)])[0][0] == [1, 0, 0]


def test_hermite_normal_form_on_designed_lattices():
    assert R.hnf([]) == ([[0, 0, 0]] * 3, 0) and R.hnf([(0, 0, 0)]) == ([[0, 0, 0]] * 3, 0)
    assert R.hnf([(-1, -2, 0)]) == ([[1, 2, 0], [0, 0, 0], [0, 0, 0]], 1)
    assert R.hnf([(0, 0, -3)]) == ([[0, 0, 3], [0, 0, 0], [0, 0, 0]], 1)
    assert R.hnf([(2, 0, 0), (0, 4, 0), (1, 2, 0)]) == ([[1, 2, 0], [0, 4, 0], [0, 0, 0]], 2)
    assert R.hnf([(2, 0, 0), (0, 3, 0), (1, 1, 0)]) == ([[1, 0, 0], [0, 1, 0], [0, 0, 0]], 2)            # (0, 3, 0) - (0, 2, 0)
    assert R.hnf([(1, 1, 1), (1, -1, 0), (0, 0, 2)]) == ([[1, 1, 1], [0, 2, 1], [0, 0, 2]], 3)
    assert R.hnf([(4, 6, 0), (6, 9, 0)]) == ([[2, 3, 0], [0, 0, 0], [0, 0, 0]], 1)                 # dependent: rank 1
    big = 1 << 31
    assert R.hnf([(big, 2 * big, 0), (3 * big, 6 * big, 0)]) == ([[big, 2 * big, 0], [0, 0, 0], [0, 0, 0]], 1)
    rng = np.random.default_rng(3)
    for _ in range(50):                                             # the form does not depend on the generators or their order
        gens = rng.integers(-9, 10, size=(4, 3)).tolist()
        mixed = [[a + 2 * b for a, b in zip(gens[0], gens[1])], gens[1], gens[3], gens[2], [-x for x in gens[0]]]
        assert R.hnf(gens) == R.hnf(mixed)
        h, rank = R.hnf(gens)
        for r in range(rank):
            c = next(k for k in range(3) if h[r][k] != 0)
            assert h[r][c] > 0 and all(0 <= h[q][c] < h[r][c] for q in range(r)) and all(h[q][c] == 0 for q in range(r + 1, 3))


def test_two_channels_have_no_component_of_rank_two():
    (case,) = [c for c in DESIGNED if c[0] == "two_channels"]
    t, r = R.levels(case[1], 26)
    assert t.tolist() == [1.0, 0.0, 0.0] and r.tolist() == [1, 0, 0]


S = 0.3                                                              # the designed saddle


def saddle_grid():
    g = np.full((5, 6, 7), 0.01)
    g[2, 3, :] = 5.0                                                 # a channel along the last axis ...
    g[2, 3, 4] = S                                                   # ... through one saddle voxel between its two basins
    return g


def test_the_saddle_value_is_the_first_level_on_its_bytes():
    g = saddle_grid()
    t, r = R.levels(g, 26)
    assert t.tobytes() == np.array([S, 0.01, 0.01]).tobytes() and r.tolist() == [1, 3, 3]
    assert R.max_rank(g, S) == 1 and R.max_rank(g, np.nextafter(S, 1.0)) == 0 and R.max_rank(g, 0.01) == 3
    assert R.snap(g, np.nextafter(0.01, 1.0)) == S and R.snap(g, S) == S and R.snap(g, 5.5) is None and R.snap(g, 1e-300) == 0.01


def test_plateaus_and_a_level_equal_to_a_value():
    g = np.zeros((4, 4, 6))
    g[1, 1, :] = 2.0                                                 # a plateau that is a channel
    g[1, 2, :3] = 3.0
    g[3, 3, 0] = 2.0
    _, _, at = summary(g, 2.0, 6)                                    # >= : the value itself is in the set
    assert at == [(9, 1, [[0, 0, 1], [0, 0, 0], [0, 0, 0]]), (1, 0, [[0, 0, 0]] * 3)]
    _, _, above = summary(g, np.nextafter(2.0, 3.0), 6)
    assert above == [(3, 0, [[0, 0, 0]] * 3)]
    assert R.levels(g, 6)[0].tolist() == [2.0, 0.0, 0.0]


def test_nan_voxels_are_never_in_the_set():
    g = np.zeros((4, 4, 6))
    g[1, 1, :] = 2.0
    g[1, 1, 3] = np.nan
    labels, _, got = summary(g, 1.0, 26)
    assert got == [(5, 0, [[0, 0, 0]] * 3)] and labels[1, 1, 3] == -1
    labels, _, got = summary(g, -np.inf, 26)                         # every number passes, the NaN does not
    assert got[0][0] == 95 and labels[1, 1, 3] == -1 and got[0][1] == 3
    assert R.levels(g, 26)[0].tolist() == [0.0, 0.0, 0.0]
    assert R.levels(np.full((3, 3, 3), np.nan))[0].tolist() == [0.0, 0.0, 0.0]


def test_all_zero_and_negative_grids_have_no_level():
    for g in (np.zeros((3, 4, 5)), -np.ones((3, 4, 5)), np.full((1, 1, 1), -0.0)):
        t, r = R.levels(g)
        assert t.tolist() == [0.0, 0.0, 0.0] and r.tolist() == [0, 0, 0]
    t, r = R.levels(np.full((1, 1, 1), 1e-310))                      # a subnormal is positive
    assert t.tolist() == [1e-310] * 3 and r.tolist() == [3, 3, 3]


def test_neighbours_and_shifts_on_axes_of_one_and_two():
    assert R.neighbour((0, 0, 0), (1, -1, 0), (1, 1, 5)) == ((0, 0, 0), (1, -1, 0))
    assert R.neighbour((1, 0, 4), (1, -1, 1), (2, 2, 5)) == ((0, 1, 0), (1, -1, 1))
    assert R.neighbour((0, 1, 2), (1, -1, 1), (2, 2, 5)) == ((1, 0, 3), (0, 0, 0))
    assert [len(R.offsets(c)) for c in (6, 18, 26)] == [6, 18, 26]
    assert R.seam_max((1, 1, 1), 6) == 3 and R.seam_max((1, 1, 1), 26) == 13 and R.seam_max((5, 6, 7), 6) == 42 + 35 + 30


def test_the_predicate_is_monotone_over_every_distinct_value():
    rng = np.random.default_rng(11)
    g = rng.integers(0, 40, size=(5, 5, 6)).astype(float) / 8.0      # 150 voxels, plateaus
    g[rng.integers(0, 5), rng.integers(0, 5), rng.integers(0, 6)] = np.nan
    for connectivity in (6, 26):
        values = np.unique(g[g > 0.0])
        ranks = [R.max_rank(g, v, connectivity) for v in values]
        assert all(a >= b for a, b in zip(ranks, ranks[1:])) and ranks[0] == 3 and ranks[-1] == 0
        t, r = R.levels(g, connectivity)
        assert t[0] >= t[1] >= t[2] > 0.0
        for d in range(3):
            assert R.max_rank(g, t[d], connectivity) == r[d] >= d + 1
            above = values[values > t[d]]
            assert len(above) == 0 or R.max_rank(g, above[0], connectivity) < d + 1
