"""CPU-only: the front of ``sitator_amd/landscape.py`` through the stub of tests/test_landscape_binding.py.  The stub's
``sit_landscape_energies`` writes a designed grid, its ``sit_density_peaks`` and ``sit_percolation_levels`` answer with the rules of
their headers restated in numpy (tests/percolation_ref.py for the levels): ``capped``, ``energies3`` and the order of the minima are
host code and are checked here on grids made for them."""
import ctypes as C

import numpy as np
import pytest

from sitator_amd import EnergyLandscape, LandscapeResult, SiteNetwork, Structure, calculators
from sitator_amd.landscape import level_energies
from tests import landscape_ref as LR
from tests import percolation_ref as PR
from tests.test_landscape_binding import LandscapeStub, make_ctx


def peaks_of(g, threshold):
    """The rule of ``sit_density_peaks``, restated."""
    n = g.shape
    out = []
    for v in range(g.size):
        i = np.unravel_index(v, n)
        if not g[i] >= threshold:
            continue
        ok = True
        for d in np.ndindex(3, 3, 3):
            u = int(np.ravel_multi_index(tuple((i[a] + d[a] - 1) % n[a] for a in range(3)), n))
            gu = g.reshape(-1)[u]
            ok &= u == v or gu < g[i] or (gu == g[i] and u > v)
        if ok:
            out.append(v)
    return out


@pytest.fixture
def stub():
    s = LandscapeStub()

    def peaks(args):
        found = peaks_of(args[1]._arr, args[3])
        out = C.cast(args[5], C.POINTER(C.c_int64))
        for k, v in enumerate(found[:args[4]]):
            out[k] = v
        args[6]._obj.value = len(found)

    def levels(args):
        t, r = PR.levels(args[1]._arr, args[3])
        args[5]._arr[:] = t
        args[6]._arr[:] = r
        args[7]._arr[:] = [7, 2, 5, 1]
    s.effects["sit_density_peaks"] = peaks
    s.effects["sit_percolation_levels"] = levels
    return s


@pytest.fixture
def ctx(stub):
    c = make_ctx(stub)
    yield c
    c._h = None


def test_compute_hands_the_static_atoms_and_their_parameters_on(stub, ctx):
    grid_values = np.arange(24, dtype=np.float64).reshape(2, 3, 4)

    def effect(args):
        args[8]._arr[...] = grid_values
        args[9]._arr[:] = [1, 1, 0, 99]
    stub.effects["sit_landscape_energies"] = effect
    cell = np.diag([4.0, 6.0, 8.0])
    pos = np.array([[0.5, 0.5, 0.5], [1.0, 2.0, 3.0], [3.0, 3.0, 3.0]])
    sn = SiteNetwork(Structure(pos, cell, numbers=[8, 3, 16]), [True, False, True], [False, True, False])
    calc = calculators.LennardJones(epsilon={8: 1.0, 16: 0.4}, sigma={8: 1.0, 16: 1.3}, rc=3.5)
    el = EnergyLandscape(calc, grid=(2, 3, 4), form=1)
    res = el.compute(sn, ctx=ctx)
    (args,) = stub.of("sit_landscape_energies")
    assert np.array_equal(args[1]._arr, pos[[0, 2]]) and args[2]._arr.tolist() == [1.0, 0.4] and args[3]._arr.tolist() == [1.0, 1.3]
    assert args[4:6] == (2, 3.5) and list(args[6]._arr) == [2, 3, 4] and args[7] == 1
    assert isinstance(res, LandscapeResult) and res.grid == (2, 3, 4) and res.e_min == 0.0 and np.array_equal(res.energies, grid_values)
    assert (res.form, res.tiles, res.list_chunks, res.candidate_terms) == (1, 1, 0, 99) and np.array_equal(res.cell, cell)
    assert EnergyLandscape(calc, spacing=0.5).grid_for(cell) == (8, 12, 16) and EnergyLandscape(calc, spacing=0.001).grid_for(cell) == (1024,) * 3
    with pytest.raises(TypeError, match="LennardJones"):
        EnergyLandscape(object())
    with pytest.raises(ValueError, match="spacing"):
        EnergyLandscape(calc, spacing=0.0)
    with pytest.raises(ValueError, match="atomic number"):
        el.compute_for_positions(pos, [8, 3, 16], cell, ctx=ctx)


def test_centres_follow_the_rule_of_the_kernels():
    cell = np.array([[4.0, 0.0, 0.0], [0.8, 3.8, 0.0], [0.5, 0.6, 3.9]])
    res = LandscapeResult(np.zeros((3, 5, 7)), cell)
    f, x = res.fractional_centers(), res.cartesian_centers()
    assert f.shape == x.shape == (3, 5, 7, 3)
    for i in ((0, 0, 0), (2, 4, 6), (1, 3, 2)):
        assert f[i].tolist() == [(i[a] + 0.5) / res.grid[a] for a in range(3)]
        assert x[i].tobytes() == LR.center(cell, res.grid, i).tobytes()


def test_capped_is_monotone_and_positive_below_the_cap():
    E = np.array([[[3.0, -1.0, np.inf, 7.0, 7.0, 2.0]]])
    res = LandscapeResult(E, np.eye(3))
    assert res.e_min == -1.0
    assert res.capped().tolist() == [[[4.0, 8.0, 0.0, 0.0, 0.0, 5.0]]]                # the default cap: the largest finite energy
    assert res.capped(3.0).tolist() == [[[0.0, 4.0, 0.0, 0.0, 0.0, 1.0]]]
    assert res.capped(100.0).tolist() == [[[97.0, 101.0, 0.0, 93.0, 93.0, 98.0]]]
    assert LandscapeResult(np.full((1, 1, 2), np.inf), np.eye(3)).capped().tolist() == [[[0.0, 0.0]]]


def channel_grid():
    """4 x 4 x 4: a channel of energy 1.0 along the last axis through a saddle of 2.0, joined to its images along the second axis
    over a saddle of 5.0 (twice: repeated values) and along the first over the same 5.0; everything else 9.0, one atom (+inf)."""
    E = np.full((4, 4, 4), 9.0)
    E[0, 0, :] = [1.0, 1.0, 2.0, 1.0]
    E[0, 1:, 0] = [5.0, 3.0, 5.0]
    E[1:, 0, 0] = [3.0, 5.0, 4.0]
    E[2, 2, 2] = np.inf
    return E


def test_energies3_on_repeated_values_and_on_an_atom(ctx):
    E = channel_grid()
    res = LandscapeResult(E, np.eye(3) * 4.0)
    p = res.percolation(ctx=ctx)
    g = res.capped()
    assert g.max() == 8.0 and g[2, 2, 2] == 0.0 and (g[E == 9.0] == 0.0).all()
    assert p.levels.tolist() == [7.0, 4.0, 4.0] and p.ranks.tolist() == [1, 3, 3] and p.dimensionality == 3
    assert p.energies3.tolist() == [2.0, 5.0, 5.0] and p.barriers3.tolist() == [1.0, 4.0, 4.0] and p.passes == 7
    # a cap below the second saddle: one dimension is left
    low = res.percolation(e_cap=4.5, ctx=ctx)
    assert low.levels.tolist() == [2.5, 0.0, 0.0] and low.energies3[0] == 2.0 and np.isnan(low.energies3[1:]).all()
    assert np.isnan(low.barriers3[1:]).all() and low.dimensionality == 1
    # nothing below the cap percolates
    none = res.percolation(e_cap=1.5, ctx=ctx)
    assert none.levels.tolist() == [0.0, 0.0, 0.0] and np.isnan(none.energies3).all()


def test_level_energies_is_the_largest_energy_of_the_superlevel_set():
    E = np.array([[[1.0, 1.0 + 2.0 ** -52, 2.0, np.inf, 2.0, 3.0]]])
    g = np.array([[[2.0, 2.0, 1.0, 0.0, 1.0, 0.0]]])              # two energies on one value of g, as a large cap rounds them
    out = level_energies(E, g, [2.0, 1.0, 0.0])
    assert out[0] == 1.0 + 2.0 ** -52 and out[1] == 2.0 and np.isnan(out[2])


def test_minima_are_sorted_by_energy_with_ties_by_index(ctx):
    E = np.full((4, 4, 6), 9.0)
    E[0, 0, 0], E[2, 2, 3], E[0, 2, 3], E[2, 0, 0] = 1.0, -2.0, 1.0, 4.0
    E[2, 0, 1] = 4.0                                                # a plateau: the lower index is the minimum
    E[1, 1, 5] = np.inf
    res = LandscapeResult(E, np.diag([4.0, 4.0, 6.0]))
    v, f, x, e = res.minima(ctx=ctx)
    flat = lambda i: (i[0] * 4 + i[1]) * 6 + i[2]                 # noqa: E731
    assert v.tolist() == [flat((2, 2, 3)), flat((0, 0, 0)), flat((0, 2, 3)), flat((2, 0, 0))] and e.tolist() == [-2.0, 1.0, 1.0, 4.0]
    assert f[0].tolist() == [2.5 / 4, 2.5 / 4, 3.5 / 6] and x[0].tolist() == [2.5, 2.5, 3.5]
    v, _, _, e = res.minima(window=3.5, ctx=ctx)                    # below e_min + 3.5 = 1.5
    assert v.tolist() == [flat((2, 2, 3)), flat((0, 0, 0)), flat((0, 2, 3))]
    v, _, _, _ = res.minima(window=0.0, ctx=ctx)
    assert len(v) == 0
    (first,) = [c for c in ctx.lib.of("sit_density_peaks")][:1]
    assert first[3] == np.nextafter(0.0, 1.0)


def test_components_level_and_cube_file(ctx, tmp_path):
    E = channel_grid()
    res = LandscapeResult(E, np.eye(3) * 4.0)
    ctx.lib.effects["sit_percolation_components"] = lambda args: None
    res.components(2.0, connectivity=6, e_cap=10.0, ctx=ctx)
    args = ctx.lib.of("sit_percolation_components")[-1]
    assert args[3] == 8.0 and args[4] == 6 and np.array_equal(args[1]._arr, res.capped(10.0))
    with pytest.raises(ValueError, match="below the cap"):
        res.components(10.0, e_cap=10.0, ctx=ctx)
    path = tmp_path / "e.cube"
    res.write_cube(str(path), structure=Structure([[0.5, 0.5, 0.5]], np.eye(3) * 4.0, numbers=[8]), e_cap=6.0)
    lines = path.read_text().splitlines()
    assert lines[2].split()[0] == "1" and [ln.split()[0] for ln in lines[3:6]] == ["4", "4", "4"] and lines[6].split()[0] == "8"
    values = np.array([float(x) for ln in lines[7:] for x in ln.split()]).reshape(4, 4, 4)
    assert np.array_equal(values, np.minimum(E, 6.0)) and values.max() == 6.0
