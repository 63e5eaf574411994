"""GPU: ``sit_landscape_energies`` (landscape.hip: the direct and the tiled kernel) and ``EnergyLandscape`` / ``LandscapeResult`` on top
of it, against the restatement of tests/landscape_ref.py (itself pinned to ``math.fsum`` and to values computed by hand by
tests/test_landscape_ref.py, and to landscape_plan.h by tests/test_landscape_plan.py).

Energies are compared on their bytes, there is no tolerance: the term is the same bits whoever evaluates it and the sum is taken in
one order.  Every case is asked of form 1, form 2, the plan's and form 1 again, and must give the same bytes on the whole grid.

The sampling rule.  The Python restatement is taken at every voxel of a grid of at most 512 voxels; on a larger grid at every voxel of
every partial tile (the tiles cut by the upper edges of the grid), at every voxel of the first full tile, and at a fixed sample (seed
5) of a tenth of all voxels: at least 10 % of the voxels of each grid are compared, which is asserted.

The shapes are the smallest at which the kernels can go wrong: one voxel, a grid inside one partial tile, partial tiles on every axis
beside full ones, whole tiles only; 1, 5, 64 and 513 atoms (one past the 512 records of the direct form's LDS tile, and two batches
and one atom of the tiled form's list); a cutoff of 0.4 and of 2.2 smallest heights of the cell - the latter on the 4 A cell with 5
atoms, where every atom has tens of images and a tile's list runs over several chunks (asserted from ``info4``)."""
import functools

import numpy as np
import pytest

from tests import barrier_ref as BR
from tests import landscape_ref as LR
from tests import percolation_ref as PR

pytestmark = pytest.mark.gpu

G1, G2, G3, G4 = (1, 1, 1), (2, 3, 5), (17, 16, 33), (8, 16, 16)
CASES = [("CUBIC", G1, 5, 0.4), ("TRICLINIC", G1, 1, 0.4), ("SMALL_TRICLINIC", G1, 5, 2.2),
         ("CUBIC", G2, 513, 0.4), ("TRICLINIC", G2, 64, 0.4), ("SMALL_TRICLINIC", G2, 1, 0.4), ("SMALL_TRICLINIC", G2, 5, 2.2),
         ("CUBIC", G3, 5, 0.4), ("TRICLINIC", G3, 64, 0.4), ("SMALL_TRICLINIC", G3, 5, 2.2),
         ("CUBIC", G4, 513, 0.4), ("TRICLINIC", G4, 1, 0.4), ("SMALL_TRICLINIC", G4, 64, 0.4), ("SMALL_TRICLINIC", G4, 5, 2.2)]


def context(cell):
    from sitator_amd import _lib
    return _lib.HipContext(np.asarray(cell, dtype=np.float64))


def device(ctx, pos, eps, sigma, rc, grid, form=0):
    from sitator_amd import _lib_landscape
    return _lib_landscape.landscape_energies(ctx, pos, eps, sigma, rc, grid, form)


def lattice(cell, S, seed):
    """S atoms at random places, every third one up to two cells outside the cell."""
    rng = np.random.default_rng(seed)
    pos = rng.random((S, 3)) @ cell
    pos[::3] += rng.integers(-2, 3, size=(len(pos[::3]), 3)) @ cell
    return pos, 0.5 + rng.random(S), 0.8 + 0.4 * rng.random(S)


def sample(grid):
    V = grid[0] * grid[1] * grid[2]
    if V <= 512:
        return np.arange(V)
    nt = LR.n_tiles(grid)
    chosen, full_taken = [np.random.default_rng(5).choice(V, size=-(-V // 10), replace=False)], False
    for t in range(nt[0] * nt[1] * nt[2]):
        vox, partial = LR.tile_voxels(grid, t)
        if partial or not full_taken:
            chosen.append(vox)
            full_taken |= not partial
    assert full_taken
    return np.unique(np.concatenate(chosen))


def check_forms(ctx, pos, eps, sigma, rc, grid):
    """Forms 1, 2, 0 and 1 again: the same bytes; returns (energies, info of form 2)."""
    nt = LR.n_tiles(grid)
    outs = [device(ctx, pos, eps, sigma, rc, grid, form) for form in (1, 2, 0, 1)]
    first = outs[0][0]
    assert first.shape == tuple(grid) and first.dtype == np.float64 and not np.isnan(first).any()
    for (e, info), form in zip(outs, (1, 2, 0, 1)):
        assert e.tobytes() == first.tobytes(), form
        assert info[0] == (form or info[0]) and info[0] in (1, 2) and info[1] == nt[0] * nt[1] * nt[2]
        assert info[3] >= 0 and (info[2] >= 0 if info[0] == 2 else info[2] == 0)
    assert outs[0][1] == outs[3][1]
    return first, outs[1][1]


@pytest.mark.parametrize("name, grid, S, rcf", CASES, ids=["%s-%s-%d-%g" % (c[0], "x".join(str(v) for v in c[1]), c[2], c[3]) for c in CASES])
def test_energies_are_the_bytes_of_the_restatement(name, grid, S, rcf):
    cell = getattr(BR, name)
    rc = rcf * BR.heights(cell).min()
    pos, eps, sigma = lattice(cell, S, 100 + S + grid[2])
    with context(cell) as ctx:
        got, tiled = check_forms(ctx, pos, eps, sigma, rc, grid)
    vox = sample(grid)
    assert 10 * len(vox) >= got.size
    want = LR.energies(cell, pos, eps, sigma, rc, grid, vox)
    flat = got.reshape(-1)[vox]
    print("%d of %d voxels restated; list chunks of the longest tile %d, candidate terms %d" % (len(vox), got.size, tiled[2], tiled[3]))
    assert flat.tobytes() == want.tobytes(), np.nonzero(flat != want)[0][:8]
    if rcf > 2:
        # tens of images of every atom; several chunks of 448 records wherever a tile holds more than the one voxel of the smallest grid
        assert S == 5 and name == "SMALL_TRICLINIC" and tiled[2] >= (2 if got.size > 1 else 1)
        assert tiled[3] >= 30 * S * tiled[1]


def test_an_atom_on_a_voxel_centre_is_plus_infinity_and_its_neighbours_are_finite():
    for cell in (BR.TRICLINIC, BR.SMALL_TRICLINIC):
        grid = (5, 9, 10)
        at = (4, 8, 3)                                               # in a partial tile
        on = LR.center(cell, grid, at)                               # the voxel-centre arithmetic itself
        pos = np.array([on + 0.37 * cell[0] + 0.21 * cell[1], on, on + 0.43 * cell[2]])
        eps, sigma, rc = [1.0, 0.7, 0.9], [1.0, 1.2, 0.8], 0.45 * BR.heights(cell).min()
        with context(cell) as ctx:
            got, _ = check_forms(ctx, pos, eps, sigma, rc, grid)
        assert got[at] == np.inf and np.isinf(got).sum() == 1
        assert got.tobytes() == LR.energies(cell, pos, eps, sigma, rc, grid).reshape(grid).tobytes()


def test_atoms_shifted_by_whole_cell_vectors_give_the_same_energies_within_the_derived_bound():
    """Bytes need not survive a shift: ``s' = s + k cell`` is rounded, and so are ``x - s'`` and ``T`` at the larger magnitudes.  With
    ``L`` the largest coordinate that enters (``|s'| + |x| + rc``) the distance vector ``d`` of a term moves by at most
    ``delta = 8 * 2^-52 * L``, ``dd`` by ``2 d delta``; ``|d phi / d dd| <= 3 eps4 (2 s6^2 + s6) / dd``, so a term moves by at most
    ``12 A delta / d`` with ``A = eps4 (s6^2 + s6)``.  A term may enter or leave at the cutoff, where ``phi`` is 0: the same figure.
    On top, the bound of a reordered sum, ``n * 2^-53 * sum |phi|``."""
    cell, grid, S = BR.TRICLINIC, (5, 9, 10), 6
    rc = 0.4 * BR.heights(cell).min()
    pos, eps, sigma = lattice(cell, S, 9)
    pos = np.random.default_rng(2).random((S, 3)) @ cell           # inside the cell
    k = np.array([[1, 0, 0], [0, -2, 1], [3, 3, -3], [0, 0, 0], [-1, 2, 0], [2, -1, -2]])
    moved = pos + k @ cell
    with context(cell) as ctx:
        base, _ = check_forms(ctx, pos, eps, sigma, rc, grid)
        shifted, _ = check_forms(ctx, moved, eps, sigma, rc, grid)
    L = np.abs(moved).max() + np.abs(np.sum(np.abs(cell), axis=0)).max() + rc
    delta = 8.0 * 2.0 ** -52 * L
    eps4, sig2, _ = BR.atom_constants(eps, sigma, rc)
    worst = 0.0
    for v in range(base.size):
        p, dd, atom, _ = LR.voxel_terms(cell, pos, eps, sigma, rc, LR.center(cell, grid, LR.unflatten(grid, v)))
        s6 = (sig2[atom] / dd) ** 3
        A = eps4[atom] * (s6 * s6 + s6)
        edge = (eps4 * ((sig2 / rc ** 2) ** 6 + (sig2 / rc ** 2) ** 3)).sum() * 27          # terms that may enter at the cutoff
        bound = 12.0 * delta * ((A / np.sqrt(dd)).sum() + edge / rc) + (len(p) + 1) * 2.0 ** -53 * np.abs(p).sum()
        diff = abs(base.reshape(-1)[v] - shifted.reshape(-1)[v])
        worst = max(worst, diff / bound if bound > 0 else (0.0 if diff == 0 else np.inf))
        assert diff <= bound, (v, diff, bound)
    print("largest |dE| / bound = %g" % worst)


def test_refusals():
    from sitator_amd import _lib, _lib_landscape
    cell = BR.SMALL_TRICLINIC
    pos, eps, sigma = lattice(cell, 3, 1)
    rc = 1.5
    with context(cell) as ctx:
        ok = functools.partial(device, ctx)
        ok(pos, eps, sigma, rc, (2, 2, 2))
        far = pos.copy()
        far[1] += np.array([2.0 ** 21, 0.0, 0.0]) @ cell
        nan = pos.copy()
        nan[2, 1] = np.nan
        for bad in (dict(form=3), dict(form=-1), dict(rc=0.0), dict(rc=-1.0), dict(rc=np.inf), dict(rc=np.nan),
                    dict(rc=256.0 * BR.heights(cell).min()), dict(eps=[1.0, -1.0, 1.0]), dict(eps=[1.0, np.inf, 1.0]), dict(sigma=[0.0, 1.0, 1.0]),
                    dict(sigma=[1.0, 1.0, np.nan]), dict(pos=far), dict(pos=nan), dict(pos=np.zeros((0, 3)), eps=[], sigma=[])):
            kw = dict(pos=pos, eps=eps, sigma=sigma, rc=rc, grid=(2, 2, 2), form=0)
            kw.update(bad)
            with pytest.raises(ValueError):
                ok(**kw)
        lib = _lib_landscape.bind(ctx.lib)                           # below the binding: the grid limits and a missing array
        out, info = np.zeros(8), np.zeros(4, dtype=np.int64)
        p, e, s = _lib._f64(pos), _lib._f64(eps), _lib._f64(sigma)

        def raw(grid, form=0, pos_ptr=_lib._d(p), out_ptr=_lib._d(out)):
            g = np.array(grid, dtype=np.int64)
            return lib.sit_landscape_energies(ctx._h, pos_ptr, _lib._d(e), _lib._d(s), 3, rc, _lib._i(g), form, out_ptr, _lib._i(info))
        assert raw((2, 2, 2)) == _lib.OK
        for grid in ((0, 2, 2), (2, 1025, 2), (2, 2, -1), (1024, 1024, 129)):
            assert raw(grid) == _lib.E_INVALID and "sit_landscape_energies" in ctx.message()
        assert raw((2, 2, 2), pos_ptr=None) == _lib.E_INVALID and raw((2, 2, 2), out_ptr=None) == _lib.E_INVALID
        assert raw((2, 2, 2), form=3) == _lib.E_INVALID
        assert lib.sit_landscape_energies(None, _lib._d(p), _lib._d(e), _lib._d(s), 3, rc, _lib._i(np.array([2, 2, 2])), 0, _lib._d(out),
                                          _lib._i(info)) == _lib.E_INVALID
        ok(pos, eps, sigma, rc, (2, 2, 2))                           # the context is as good as before
    for bad in (dict(grid=(0, 4, 4)), dict(grid=(4, 4, 4), form=5), dict(grid=(4, 4, 4), rc=0.0)):
        kw = dict(cell=cell, rc=rc, form=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            _lib_landscape.landscape_plan(**kw)


# ---- the designed host ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def designed():
    """The tetragonal host on the device (both forms) and restated, once for the tests below."""
    from sitator_amd import EnergyLandscape, calculators
    cell, pos, numbers, grid = LR.tetragonal_host()
    calc = calculators.LennardJones(epsilon=LR.TET_EPS, sigma=LR.TET_SIGMA, rc=LR.TET_RC)
    results = [EnergyLandscape(calc, grid=grid, form=form).compute_for_positions(pos, numbers, cell) for form in (1, 2)]
    want = LR.energies(cell, pos, np.full(8, LR.TET_EPS), np.full(8, LR.TET_SIGMA), LR.TET_RC, grid).reshape(grid)
    want.flags.writeable = False
    return results, want, calc


E_CAP, WINDOW = 50.0, 1.0              # above the narrow saddle (29.1); the wide saddle lies 0.31 above the minima


def test_designed_energies_in_both_forms(designed):
    results, want, _ = designed
    for res, form in zip(results, (1, 2)):
        assert res.form == form and res.grid == LR.TET_GRID and res.energies.tobytes() == want.tobytes()
        assert res.e_min == want.min() and np.isinf(res.energies).sum() == 8
        x = res.cartesian_centers()
        for i in ((0, 0, 0), (7, 3, 5), (2, 2, 2)):
            assert x[i].tobytes() == LR.center(res.cell, res.grid, i).tobytes()


def test_designed_minima_are_the_eight_body_centres(designed):
    results, want, _ = designed
    body, wide, _ = LR.tetragonal_voxels()
    assert want.reshape(-1)[wide].min() - want.min() < WINDOW < 2.0
    v, f, x, e = results[0].minima(window=WINDOW)
    assert sorted(v.tolist()) == body.tolist() and e.tobytes() == want.reshape(-1)[v].tobytes()
    assert np.all(np.diff(e) >= 0) and all(e[k] < e[k + 1] or v[k] < v[k + 1] for k in range(7))
    for k in range(8):
        assert x[k].tobytes() == LR.center(results[0].cell, LR.TET_GRID, LR.unflatten(LR.TET_GRID, int(v[k]))).tobytes()
    assert len(results[0].minima()[0]) >= 8                         # without a window: whatever else is a local minimum, too


def test_designed_percolation_levels_energies_and_components(designed):
    results, want, _ = designed
    res = results[1]
    body, wide, narrow = LR.tetragonal_voxels()
    flat = want.reshape(-1)
    p = res.percolation(e_cap=E_CAP)
    g = res.capped(E_CAP)
    assert g.tobytes() == np.where(want < E_CAP, E_CAP - want, 0.0).tobytes()
    t, r = PR.levels(g, 26)
    assert p.levels.tobytes() == t.tobytes() and np.array_equal(p.ranks, r)
    # along c through the wide a x a windows first, the two other directions together
    assert p.levels[0] > p.levels[1] == p.levels[2] > 0.0 and p.ranks.tolist() == [1, 3, 3] and p.dimensionality == 3
    assert p.energies3[0].tobytes() in {flat[v].tobytes() for v in wide}
    assert p.energies3[1].tobytes() in {flat[v].tobytes() for v in narrow} and p.energies3[2].tobytes() == p.energies3[1].tobytes()
    assert np.array_equal(p.barriers3, p.energies3 - want.min())
    # between the two saddles: four channels along c
    between = 0.5 * (flat[wide].max() + flat[narrow].min())
    comp = res.components(between, e_cap=E_CAP)
    labels, roots, sizes, rank, basis = PR.components(g, E_CAP - between, 26)
    assert comp.labels.tobytes() == labels.tobytes() and np.array_equal(comp.roots, roots) and np.array_equal(comp.sizes, sizes)
    assert np.array_equal(comp.rank, rank) and np.array_equal(comp.basis, basis)
    assert rank.tolist() == [1, 1, 1, 1] and all(b.tolist() == [[0, 0, 1], [0, 0, 0], [0, 0, 0]] for b in basis)


def test_designed_match_sites(designed):
    from sitator_amd import SiteNetwork, Structure
    results, want, _ = designed
    cell, pos, numbers, grid = LR.tetragonal_host()
    body, _, _ = LR.tetragonal_voxels()
    centers = np.array([LR.center(cell, grid, LR.unflatten(grid, int(v))) for v in body])
    structure = Structure(np.concatenate([pos, centers[:1]]), cell, numbers=list(numbers) + [3])
    sn = SiteNetwork(structure, np.arange(9) < 8, np.arange(9) == 8)
    sn.centers = centers
    m = results[0].match_sites(sn, window=WINDOW)
    assert m["site_energy"].tobytes() == want.reshape(-1)[body].tobytes()
    assert m["site_minimum_distance"].tolist() == [0.0] * 8 and m["minimum_site_distance"].tolist() == [0.0] * 8
    assert sorted(m["minimum_voxels"][m["site_minimum"]].tolist()) == body.tolist()
    assert m["minimum_voxels"][m["site_minimum"]].tolist() == body.tolist()
    # compute(sn) takes the static atoms, their numbers and the cell from the network
    from sitator_amd import EnergyLandscape
    again = EnergyLandscape(designed[2], grid=grid).compute(sn)
    assert again.energies.tobytes() == want.tobytes()
