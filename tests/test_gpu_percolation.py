"""GPU: ``sit_percolation_components`` and ``sit_percolation_levels`` (percolation.hip: the tile-local labelling in LDS, the global
rounds, the seam records and the quotient step, the relabelling, sizes and compacted roots, the bisection for the levels) and
``density_components`` / ``density_percolation`` / ``DensityResult.components`` / ``.percolation`` on top of them, against the
restatement of tests/percolation_ref.py (itself pinned to designed answers by tests/test_percolation_ref.py and to percolation_plan.h
by tests/test_percolation_plan.py).

Labels, roots, sizes, ranks and bases are integers and a level is the bytes of a voxel's value: everything is compared on its
bytes, there is no tolerance.  Every case is asked of both labelling forms, and once more, and must give the same bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import msd_ref as M
from tests import percolation_ref as R
from tests.test_gpu_msd import Context
from tests.test_percolation_ref import S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 3, 5), (17, 16, 33), (64, 48, 40)]
# site-percolation thresholds of the simple cubic lattice with 6, 18 and 26 neighbours
THRESHOLD = {6: 0.3116, 18: 0.1372, 26: 0.0976}


def same_bytes(got, exp):
    return got is not None and got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()


def device_components(ctx, grid, level, connectivity, form=0):
    from sitator_amd import _lib_percolation
    return _lib_percolation.percolation_components(ctx, grid, level, connectivity, form)


def check_components(ctx, grid, level, connectivity, exp=None, forms=(1, 2, 0, 2)):
    """Both forms, the plan's, and one of them again: the restatement's bytes every time."""
    exp = exp or R.components(grid, level, connectivity)
    labels, roots, sizes, rank, basis = exp
    info = None
    for form in forms:
        got_labels, rec, info = device_components(ctx, grid, level, connectivity, form)
        assert same_bytes(got_labels, labels), (grid.shape, level, connectivity, form)
        assert rec.shape == (len(roots), 12) and rec.dtype == np.int64
        assert np.array_equal(rec[:, 0], roots) and np.array_equal(rec[:, 1], sizes) and np.array_equal(rec[:, 2], rank)
        assert np.array_equal(rec[:, 3:].reshape(-1, 3, 3), basis)
        assert info[0] >= 1 and 0 <= info[3] <= info[1] <= R.seam_max(grid.shape, connectivity) and info[2] == (form or info[2])
    return info


def embed(shape, voxels, value=1.0, base=0.0):
    g = np.full(shape, base)
    for v in voxels:
        g[tuple(int(x) % n for x, n in zip(v, shape))] = value
    return g


def double_loop(shape, at):
    """The double loop of tests/percolation_ref.py along the first axis of any length >= 8, its two strands at the transverse offset
    ``at`` (positions are taken modulo the grid: an offset near a face puts the strands across it)."""
    n0 = shape[0]
    a = [R.STRAND_A[0]] * (n0 - 8) + R.STRAND_A
    b = [R.STRAND_B[0]] * (n0 - 8) + R.STRAND_B
    return embed(shape, [(i, at[0] + p[0], at[1] + p[1]) for i in range(n0) for p in (a[i], b[i])])


def saddle(shape, at, k, background=0.01):
    """A channel of 5.0 along the last axis at ``at`` through one voxel of value S at index ``k``, over a background."""
    g = np.full(shape, background)
    g[at[0], at[1], :] = 5.0
    g[at[0], at[1], k] = S
    return g


def thin_serpentine(shape):
    """One path, a voxel wide, that only its consecutive voxels connect under 6 neighbours: every other row of every other plane, joined
    at alternating ends.  The longest label chain a grid of this size can hold."""
    n0, n1, n2 = shape
    g = np.zeros(shape)
    planes, rows = range(0, n0 - 2, 2), range(0, n1 - 1, 2)
    step, at_end = 0, False
    for a, i in enumerate(planes):
        order = list(rows) if a % 2 == 0 else list(rows)[::-1]
        for b, j in enumerate(order):
            ks = range(n2 - 1) if not at_end else range(n2 - 2, -1, -1)
            for k in ks:
                step += 1
                g[i, j, k] = step
            at_end = not at_end
            k_end = n2 - 2 if at_end else 0
            if b + 1 < len(order):
                step += 1
                g[i, (j + order[b + 1]) // 2, k_end] = step
            elif a + 1 < len(planes):
                step += 1
                g[i + 1, j, k_end] = step
    return g


def full_serpentine(shape):
    """A path that visits every voxel exactly once, the value of a voxel its place on the path."""
    n0, n1, n2 = shape
    g = np.zeros(shape)
    step = 0
    for i in range(n0):
        for jj in range(n1):
            j = jj if i % 2 == 0 else n1 - 1 - jj
            ks = range(n2) if (i * n1 + jj) % 2 == 0 else range(n2 - 1, -1, -1)
            for k in ks:
                step += 1
                g[i, j, k] = step
    return g


@functools.lru_cache(maxsize=None)
def designed_on(shape):
    """``{name: (grid, level, connectivity)}``: channels, planes, loops and saddles across the tile faces (8, 8, 16) and the cell faces of
    ``shape``."""
    n0, n1, n2 = shape
    out = {}
    for a in range(3):
        fixed = [7 % n0, 8 % n1, 16 % n2]
        line = [tuple(k if b == a else fixed[b] for b in range(3)) for k in range(shape[a])]
        out["channel_along_%d" % a] = (embed(shape, line), 1.0, 6)
    out["plane_on_a_tile_face"] = (embed(shape, [(8 % n0, j, k) for j in range(n1) for k in range(n2)]), 1.0, 6)
    out["full"] = (np.ones(shape), 1.0, 18)
    out["two_channels"] = (embed(shape, [(i, 1 % n1, 1 % n2) for i in range(n0)] + [(3 % n0, j, (n2 // 2 + 1) % n2) for j in range(n1)]), 0.5, 26)
    for connectivity in (6, 18, 26):
        out["space_diagonal_%d" % connectivity] = (embed(shape, [(t, t, t) for t in range(n0 * n1 * n2)][:4 * max(shape)]), 1.0, connectivity)
    if n0 >= 8 and n1 >= 5 and n2 >= 5:
        out["double_loop_across_a_tile_face"] = (double_loop(shape, (5, 13)), 1.0, 26)
        out["double_loop_across_the_cell_faces"] = (double_loop(shape, (n1 - 2, n2 - 3)), 1.0, 18)
    out["saddle_on_a_tile_face"] = (saddle(shape, (8 % n0, 7 % n1), 16 % n2), S, 26)
    out["above_the_saddle"] = (saddle(shape, (8 % n0, 7 % n1), 16 % n2), float(np.nextafter(S, 1.0)), 26)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_designed_grids_across_tile_and_cell_faces(shape):
    with Context(M.ORTHO) as ctx:
        for name, (grid, level, connectivity) in designed_on(shape).items():
            check_components(ctx, grid, level, connectivity, forms=(1, 2))


def test_designed_answers_on_the_device():
    """Not through the restatement: the answers tests/test_percolation_ref.py reads off."""
    with Context(M.ORTHO) as ctx:
        for name, grid, level, connectivity, expected in R.designed():
            for form in (1, 2):
                _, rec, _ = device_components(ctx, grid, level, connectivity, form)
                got = [(int(r[1]), int(r[2]), r[3:].reshape(3, 3).tolist()) for r in rec]
                assert got == expected, (name, form)
        rec = device_components(ctx, double_loop((17, 16, 33), (6, 14)), 1.0, 26)[1]
        assert len(rec) == 1 and rec[0, 1] == 34 and rec[0, 2] == 1 and rec[0, 3:6].tolist() == [2, 0, 0]


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_random_fields_at_three_fill_fractions(shape, connectivity):
    rng = np.random.default_rng(100 + connectivity + shape[0])
    field = rng.random(shape)
    pc = THRESHOLD[connectivity]
    with Context(M.ORTHO) as ctx:
        for fill in (0.5 * pc, pc, 0.8):                             # sparse, near the threshold, dense
            check_components(ctx, field, 1.0 - fill, connectivity, forms=(1, 2, 0, 2) if field.size < 10000 else (1, 2))


@pytest.mark.parametrize("shape", [(64, 48, 40), (64, 48, 44)], ids=str)
def test_checkerboard_has_a_component_per_voxel(shape):
    """Under 6 neighbours no two voxels of one colour touch: V / 2 components of one voxel.  On the second grid they are more than the
    first request of the record protocol has room for."""
    idx = np.indices(shape).sum(axis=0)
    grid = (idx % 2 == 0).astype(np.float64)
    V = grid.size
    roots = np.flatnonzero(grid.reshape(-1)).astype(np.int32)
    labels = np.where(grid.reshape(-1) > 0, np.arange(V), -1).astype(np.int32).reshape(shape)
    exp = (labels, roots, np.ones(V // 2, dtype=np.int64), np.zeros(V // 2, dtype=np.int32), np.zeros((V // 2, 3, 3), dtype=np.int32))
    assert len(roots) == V // 2 and (len(roots) > 1 << 16) == (shape[2] == 44)
    with Context(M.ORTHO) as ctx:
        info = check_components(ctx, grid, 0.5, 6, exp=exp, forms=(1, 2))
        assert info[0] == 2 and info[1] == 0                         # the tile form's two rounds find nothing to hook; no seam edge in the set
        assert device_components(ctx, grid, 0.5, 6, 1)[2][0] == 1
        # ... and with 26 neighbours it is one component that fills the cell
        _, rec, _ = device_components(ctx, grid, 0.5, 26)
        assert rec.tolist() == [[0, V // 2, 3, 1, 0, 0, 0, 1, 0, 0, 0, 1]]


def test_serpentines_on_17_16_33():
    shape = SHAPES[2]
    thin = thin_serpentine(shape)
    length = int((thin > 0).sum())
    assert length > 2000 and thin.max() == length
    every = full_serpentine(shape)
    assert np.array_equal(np.sort(every.reshape(-1)), np.arange(1, every.size + 1))
    with Context(M.ORTHO) as ctx:
        info = check_components(ctx, thin, 1.0, 6)
        exp = R.components(thin, 1.0, 6)
        assert len(exp[1]) == 1 and exp[2][0] == length and exp[3][0] == 0     # one open path
        assert info[0] >= 2
        check_components(ctx, thin, float(length // 2), 6, forms=(1, 2))       # its second half
        check_components(ctx, thin, 1.0, 26, forms=(1, 2))
        check_components(ctx, every, 1.0, 6, forms=(1, 2))                     # every voxel: the cell
        check_components(ctx, every, float(every.size // 2), 6, forms=(1, 2))  # the second half of the path: a slab


def test_nan_and_negative_values():
    rng = np.random.default_rng(12)
    grid = rng.normal(size=SHAPES[2])
    grid.reshape(-1)[rng.integers(0, grid.size, 300)] = np.nan
    grid[3, 4, 5], grid[3, 4, 6] = np.inf, -np.inf
    with Context(M.ORTHO) as ctx:
        for level in (-np.inf, -0.5, 0.0, 1.0, np.inf):
            check_components(ctx, grid, level, 26, forms=(1, 2))
        labels = device_components(ctx, grid, -np.inf, 6)[0]
        assert np.array_equal(labels < 0, np.isnan(grid))            # every number passes -inf, no NaN does
        only_nan = np.full((5, 4, 3), np.nan)
        labels, rec, _ = device_components(ctx, only_nan, -np.inf, 26)
        assert np.all(labels == -1) and rec.shape == (0, 12)


def device_levels(ctx, grid, connectivity, form=0):
    from sitator_amd import _lib_percolation
    return _lib_percolation.percolation_levels(ctx, grid, connectivity, form)


def check_levels(ctx, grid, connectivity):
    exp_t, exp_r = R.levels(grid, connectivity)
    for form in (1, 2, 0):
        t, r, info = device_levels(ctx, grid, connectivity, form)
        assert t.tobytes() == exp_t.tobytes() and same_bytes(r, exp_r), (grid.shape, connectivity, form, t, exp_t)
        assert info[0] <= 3 * 64 and (info[0] > 0) == bool(np.any(grid > 0.0))
    return exp_t, exp_r


def test_levels_are_the_restatement():
    rng = np.random.default_rng(5)
    palette = np.sort(rng.random(24) ** 6 * 1e3)                     # 24 doubles over many binades: the bytes of a level are one of them
    quantised = palette[rng.integers(0, 24, size=SHAPES[2])]
    small = [np.zeros((3, 4, 5)), -np.ones((2, 2, 2)), np.full((1, 1, 1), 1e-310), np.full((1, 1, 1), 3.5), np.full((2, 3, 1), np.nan),
             rng.random(SHAPES[1]), rng.random(SHAPES[1]) * 1e-300, np.where(rng.random((7, 6, 5)) < 0.3, np.inf, rng.random((7, 6, 5)))]
    with Context(M.ORTHO) as ctx:
        for g in small:
            for connectivity in (6, 18, 26):
                check_levels(ctx, g, connectivity)
        for connectivity in (6, 26):
            t, r = check_levels(ctx, quantised, connectivity)
            assert t[0] >= t[1] >= t[2] > 0.0 and all(v in palette for v in t)
        t, r = check_levels(ctx, saddle(SHAPES[2], (8, 7), 16), 26)
        assert t.tobytes() == np.array([S, 0.01, 0.01]).tobytes() and r.tolist() == [1, 3, 3]
        # the largest grid: a channel through a saddle, a plane below it, nothing that fills the cell
        big = saddle(SHAPES[3], (8, 7), 16, background=0.0)
        big[40, :, :] = 0.2
        t, r = check_levels(ctx, big, 6)
        assert t.tobytes() == np.array([S, 0.2, 0.0]).tobytes() and r.tolist() == [1, 2, 0]
        for name, (grid, _, connectivity) in designed_on(SHAPES[2]).items():
            if name != "full":
                check_levels(ctx, grid, connectivity)


def test_limits_are_errors_not_faults():
    from sitator_amd import _lib, _lib_percolation
    ok = np.random.default_rng(1).random((4, 5, 6))
    with Context(M.ORTHO) as ctx:
        exp = R.components(ok, 0.5, 26)
        for bad in (dict(grid=np.zeros((0, 4, 4))), dict(grid=np.zeros((4, 1025, 1))), dict(grid=np.zeros((1024, 1024, 129))),
                    dict(connectivity=0), dict(connectivity=8), dict(connectivity=27), dict(connectivity=-6), dict(level=np.nan),
                    dict(form=3), dict(form=-1)):
            args = dict(dict(grid=ok, level=0.5, connectivity=26, form=0), **bad)
            with pytest.raises(ValueError):
                device_components(ctx, args["grid"], args["level"], args["connectivity"], args["form"])
            if "level" not in bad:
                with pytest.raises(ValueError):
                    device_levels(ctx, args["grid"], args["connectivity"], args["form"])
        lib = _lib_percolation.bind(ctx.lib)                         # a negative cap: below the binding
        n, info, g3 = C.c_int64(0), np.zeros(4, dtype=np.int64), np.array(ok.shape, dtype=np.int64)
        rec = np.zeros((4, 12), dtype=np.int64)
        assert lib.sit_percolation_components(ctx._h, _lib._d(ok), _lib._i(g3), 0.5, 26, 0, None, -1, _lib._i(rec), C.byref(n), _lib._i(info)) == _lib.E_INVALID
        # a cap of 0 and no records: the number of components alone; a cap below it: the first ones
        assert lib.sit_percolation_components(ctx._h, _lib._d(ok), _lib._i(g3), 0.5, 26, 0, None, 0, None, C.byref(n), _lib._i(info)) == _lib.OK
        assert n.value == len(exp[1])
        assert same_bytes(device_components(ctx, ok, 0.5, 26)[0], exp[0])          # and the context still works
        with pytest.raises(ValueError):
            _lib_percolation.percolation_plan((4, 4, 4), connectivity=5)


def test_operator_on_the_density_an_analysis_left_resident():
    from sitator_amd import ComponentsResult, IonicDensity, PercolationResult, density_components, density_percolation
    from tests.test_gpu_density import analysis
    la, st, frames, cell, sm, mm = analysis()
    ctx = la._ctx
    version = ctx.labels_version
    dens = IonicDensity(grid=(12, 11, 13), sigma=0.8, cutoff=3.0).compute_for_analysis(la)
    grid = dens._plane(None)
    exp_t, exp_r = R.levels(grid, 26)
    res = dens.percolation(ctx=ctx)
    own = dens.percolation()                                         # a context of its own
    free = density_percolation(grid, cell, ctx=ctx)
    for r in (res, own, free):
        assert isinstance(r, PercolationResult) and r.levels.tobytes() == exp_t.tobytes() and same_bytes(r.ranks, exp_r)
        assert r.dimensionality == int((exp_t > 0).sum()) and r.passes >= 1 and r.top == grid.max()
    kT = 0.0257
    b = res.barriers(kT)
    for d in range(3):
        assert b[d] == (np.inf if exp_t[d] == 0.0 else -kT * np.log(exp_t[d] / grid.max()))
    assert b[0] >= 0.0
    # the components at the first level (the whole support where nothing percolates): the percolating one is there
    level = float(exp_t[0]) if exp_t[0] > 0.0 else float(grid[grid > 0.0].min())
    labels, roots, sizes, rank, basis = R.components(grid, level, 26)
    comp = dens.components(level, ctx=ctx)
    for r in (comp, dens.components(level), density_components(grid, cell, level, ctx=ctx)):
        assert isinstance(r, ComponentsResult) and same_bytes(r.labels, labels) and same_bytes(r.roots, roots)
        assert same_bytes(r.sizes, sizes) and same_bytes(r.rank, rank) and same_bytes(r.basis, basis)
    assert comp.rank.max() == R.max_rank(grid, level, 26) >= (1 if exp_t[0] > 0.0 else 0) and comp.grid == (12, 11, 13)
    assert np.array_equal(comp.directions, basis.astype(np.float64) @ cell)
    flat = labels.reshape(-1)
    mass = dict.fromkeys(roots.tolist(), 0.0)
    for lab, value in zip(flat.tolist(), grid.reshape(-1).tolist()):   # one sum per component, in the order of the voxels
        if lab >= 0:
            mass[lab] += value
    assert comp.mass.tolist() == [mass[r] for r in roots.tolist()]
    for d in (1, 2, 3):
        assert np.array_equal(comp.percolating(d), np.isin(labels, roots[rank >= d]))
    assert comp.percolating(1).any() == bool(exp_t[0] > 0.0)
    # one plane, another connectivity
    split = IonicDensity(grid=(12, 11, 13), sigma=0.8, cutoff=3.0).compute_for_trajectory(la, st)
    plane0 = split._plane(0)
    t0, r0 = R.levels(plane0, 6)
    p0 = split.percolation(connectivity=6, plane=0, ctx=ctx)
    assert p0.levels.tobytes() == t0.tobytes() and same_bytes(p0.ranks, r0)
    c0 = split.components(float(plane0.max()) * 0.05, connectivity=6, plane=0, ctx=ctx)
    e0 = R.components(plane0, float(plane0.max()) * 0.05, 6)
    assert same_bytes(c0.labels, e0[0]) and same_bytes(c0.rank, e0[3])
    # the sites: the label of the voxel of every site centre, and whether that component percolates
    sn = st.site_network
    for r, lab in ((comp, labels), (c0, e0[0])):
        site_label, on_path = r.sites(sn)
        v = dens.voxel_of(np.asarray(sn.centers))
        assert np.array_equal(site_label, lab.reshape(-1)[v]) and site_label.dtype == np.int32
        table = dict(zip(r.roots.tolist(), r.rank.tolist()))
        assert on_path.tolist() == [table.get(int(x), 0) >= 1 for x in site_label]
    # nothing moved
    assert ctx.labels_version == version
