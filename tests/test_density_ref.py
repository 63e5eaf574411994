"""CPU-only: the numpy restatement of the ionic density (tests/density_ref.py) against designed inputs whose answers are known
without it, and the host parts of ``sitator_amd/density.py`` (``gaussian_stencil``, ``DensityResult``) against the restatement."""
import numpy as np
import pytest

from sitator_amd import density as D
from tests import density_ref as R
from tests import msd_ref as M

U = R.U
CUBIC = np.eye(3) * 6.0


def test_a_point_on_a_voxel_boundary_goes_to_the_upper_voxel():
    for n in (1, 3, 7, 8, 1024):
        k = np.arange(n)
        s = k / np.float64(n)                                      # f n is a whole number where k / n * n rounds back to k
        exact = (s * n) == k
        assert exact.sum() >= 0.9 * n
        got = R.axis_index(s, n)
        assert np.array_equal(got[exact], k[exact])
        below = R.axis_index(np.nextafter(s[1:], -np.inf), n)      # and just below the face: the lower one
        assert np.all(below[exact[1:]] == k[1:][exact[1:]] - 1)
    # a power-of-two grid: every boundary is exact, also shifted by whole cells
    k = np.arange(8)
    for shift in (0.0, 1.0, -3.0, 1000.0):
        assert np.array_equal(R.axis_index(k / 8.0 + shift, 8), k)


@pytest.mark.parametrize("n", [1, 3, 7, 1024])
def test_the_last_voxel_never_index_n(n):
    s = np.array([-1e-17, 1.0 - 2.0 ** -53, -2.0 ** -60, 5.0 - 2.0 ** -50, -0.0, 0.0])
    got = R.axis_index(s, n)
    assert list(got[:4]) == [n - 1] * 4 and list(got[4:]) == [0, 0]
    assert (-1e-17) - np.floor(-1e-17) == 1.0                      # f == 1.0: the product is n itself
    rng = np.random.default_rng(n)
    many = R.axis_index(np.concatenate([rng.uniform(-3, 3, 20000), -10.0 ** -rng.uniform(10, 300, 2000)]), n)
    assert many.min() >= 0 and many.max() <= n - 1
    assert list(R.axis_index(np.array([np.nan, np.inf, -np.inf]), n)) == [-1, -1, -1]


@pytest.mark.parametrize("name", sorted(M.CELLS))
def test_counts_total_and_a_cell_vector_changes_nothing(name):
    cell = M.CELLS[name]
    rng = np.random.default_rng(3)
    F, A = 23, 9
    frac = rng.integers(0, 1 << 10, size=(F, A, 3)) / float(1 << 10)
    x = frac @ cell
    x[4, 2, 1] = np.nan
    x[7, 5, 0] = np.inf
    atoms = np.array([0, 2, 5, 8])
    for grid in ((1, 1, 1), (2, 3, 5), (7, 4, 9)):
        for stride in (1, 3, 40):
            c, taken, skipped = R.counts(x, cell, atoms, grid, stride)
            assert taken == len(range(0, F, stride)) and int(c.sum()) + skipped == taken * len(atoms)
            assert c.dtype == np.uint64 and c.shape == (1,) + grid
            assert skipped == sum(1 for t in (4, 7) if t % stride == 0)
    if name == "ortho":                                            # a diagonal cell: adding whole cell vectors is exact enough
        cell2 = np.diag([8.0, 4.0, 16.0])
        y = (rng.integers(0, 1 << 22, size=(F, A, 3)) / float(1 << 20)) % np.diag(cell2)
        moved = y + rng.integers(-1000, 1001, size=(F, A, 3)) * np.diag(cell2)
        a = R.counts(y, cell2, atoms, (8, 4, 16))[0]
        assert np.array_equal(a, R.counts(moved, cell2, atoms, (8, 4, 16))[0]) and a.sum() == F * len(atoms)
        assert np.array_equal(a, R.counts(y + cell2[1], cell2, atoms, (8, 4, 16))[0])


def test_classes():
    sc = np.array([0, 2, 1, 0], dtype=np.int32)
    assert list(R.plane([-1, 0, 1, 2, 3], sc, 4)) == [3, 0, 2, 1, 0]
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 6, size=(10, 3, 3))
    labels = rng.integers(-1, 4, size=(10, 3))
    c, taken, skipped = R.counts(x, CUBIC, [0, 1, 2], (3, 3, 3), 1, labels, sc, 4)
    one = R.counts(x, CUBIC, [0, 1, 2], (3, 3, 3))[0]
    assert np.array_equal(c.sum(axis=0, keepdims=True), one) and c[3].sum() == (labels < 0).sum()
    assert c[0].sum() == np.isin(labels, [0, 3]).sum() and skipped == 0 and taken == 10


def test_smoothing_one_tap_and_the_sum_bound():
    rng = np.random.default_rng(7)
    c = rng.integers(0, 1000, size=(2, 5, 6, 7)).astype(np.uint64)
    one = R.smooth(c, [[0, 0, 0]], [1.0])
    assert one.dtype == np.float64 and np.array_equal(one, c.astype(np.float64))
    shifted = R.smooth(c, [[1, -2, 3]], [1.0])
    assert shifted[1, 0, 0, 0] == c[1, 1, 4, 3] and shifted[0, 4, 1, 6] == c[0, 0, 5, 2]
    for cell, grid, sigma in ((CUBIC, (11, 11, 11), 0.6), (M.HEX, (9, 9, 7), 0.45)):
        c = rng.integers(0, 50, size=(1,) + grid).astype(np.uint64)
        taps, w = D.gaussian_stencil(cell, grid, sigma, 3.0)
        n = len(taps)
        assert n > 20
        s = R.smooth(c, taps, w)
        total = float(c.sum())
        assert abs(float(np.sum(s.astype(np.longdouble))) - total * float(np.sum(w.astype(np.longdouble)))) <= n * U * total


@pytest.mark.parametrize("cell,grid,sigma,cutoff", [(CUBIC, (30, 30, 30), 0.31, 4.0), (M.HEX, (20, 20, 16), 0.31, 3.0),
                                                    (M.TRICLINIC, (23, 21, 22), 0.25, 4.0)])
def test_gaussian_stencil_is_the_brute_force_enumeration(cell, grid, sigma, cutoff):
    taps, w = D.gaussian_stencil(cell, grid, sigma, cutoff)
    rt, rw = R.gaussian_stencil(cell, grid, sigma, cutoff)
    assert taps.dtype == np.int64 and w.dtype == np.float64 and np.array_equal(taps, rt) and len(taps) > 27
    assert [tuple(t) for t in taps] == sorted(tuple(t) for t in taps)                   # lexicographic
    np.testing.assert_allclose(w, rw, rtol=1e-13)
    assert abs(float(np.sum(w.astype(np.longdouble))) - 1.0) <= len(w) * U
    steps = cell / np.asarray(grid, dtype=float)[:, None]
    assert np.linalg.norm(taps @ steps, axis=1).max() <= cutoff * sigma
    centre = np.where((taps == 0).all(axis=1))[0]
    assert len(centre) == 1 and w[centre[0]] == w.max() and np.array_equal(taps, -taps[::-1])


def test_gaussian_stencil_refusals():
    with pytest.raises(ValueError):
        D.gaussian_stencil(CUBIC, (4, 4, 4), 0.8)                   # 3.2 A at 1.5 A a voxel: 2 voxels, beyond (4 - 1) // 2
    assert len(D.gaussian_stencil(CUBIC, (4, 4, 4), 0.5)[0]) == 7   # 2.0 A: the centre and its six neighbours
    with pytest.raises(ValueError):
        D.gaussian_stencil(CUBIC, (200, 200, 200), 0.5)             # more than 2^15 taps
    with pytest.raises(ValueError):
        D.gaussian_stencil(CUBIC, (30, 30, 30), 0.0)
    taps, w = D.gaussian_stencil(CUBIC, (3, 3, 3), 0.1)             # the centre alone
    assert taps.tolist() == [[0, 0, 0]] and w.tolist() == [1.0]


def test_peaks():
    g = np.zeros((9, 8, 7))
    g[2, 2, 2], g[2, 2, 3], g[6, 5, 1], g[6, 6, 1] = 5.0, 3.0, 4.0, 1.0                 # two blobs
    assert list(R.peaks(g, 0.5)) == [(2 * 8 + 2) * 7 + 2, (6 * 8 + 5) * 7 + 1]
    flat = np.zeros((6, 6, 6))
    flat[1:3, 1:3, 1:3] = 2.0                                       # a plateau: its lowest-index voxel
    assert list(R.peaks(flat, 1.0)) == [(1 * 6 + 1) * 6 + 1]
    assert list(R.peaks(np.zeros((4, 5, 3)), 0.0)) == [0]           # all equal: voxel 0 only
    assert list(R.peaks(np.zeros((4, 5, 3)), 1e-300)) == []
    nan = np.zeros((5, 5, 5))
    nan[2, 2, 2] = np.nan
    nan[0, 0, 0] = 1.0
    assert list(R.peaks(nan, 0.5)) == [0] and list(R.peaks(np.full((3, 3, 3), np.nan), 0.0)) == []
    nan[1, 1, 1] = 7.0                                              # beside the NaN no comparison holds; and it tops voxel 0
    assert list(R.peaks(nan, 0.5)) == []
    wrap = np.zeros((5, 5, 5))
    wrap[0, 0, 0], wrap[4, 4, 4] = 2.0, 3.0                         # neighbours through the faces
    assert list(R.peaks(wrap, 1.0)) == [124]
    for shape in ((1, 1, 1), (2, 2, 2), (1, 2, 3), (3, 1, 2), (3, 3, 3)):   # axes of up to three voxels: everybody is everybody's neighbour
        v = np.random.default_rng(sum(shape)).integers(0, 3, size=shape).astype(float)
        assert list(R.peaks(v, 0.0)) == [int(np.argmax(v.reshape(-1)))]     # the first maximum alone
    assert list(R.peaks(np.array([[[1.0, 0.0, 1.0, 0.0, 0.5]]]), 0.6)) == [0, 2]        # (1, 1, 5): 0 and 2 are no neighbours
    assert list(R.peaks(np.array([[[1.0, 0.0, 0.0, 0.0, 1.0]]]), 0.6)) == [0]           # ... but 0 and 4 are
    assert list(R.peaks(np.array([[[1.0, 2.0], [0.0, 0.0], [0.0, 0.0], [2.0, 0.0]]]), 0.6)) == [1]   # (1, 4, 2): 1 and 6 are neighbours
    assert list(R.peaks(np.array([[[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]]), 0.6)) == [0, 3]


def result_of(counts, cell, n_frames=10, smoothed=None, names=None):
    return D.DensityResult(counts, n_frames, 0, cell, smoothed, names or ["p%d" % k for k in range(len(counts))])


def test_write_cube_reads_back(tmp_path):
    rng = np.random.default_rng(11)
    cell = M.TRICLINIC
    counts = rng.integers(0, 40, size=(2, 3, 4, 7)).astype(np.uint64)
    res = result_of(counts, cell)
    from sitator_amd import Structure
    st = Structure(np.array([[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]]), cell, [3, 8])
    for plane in (None, 1):
        path = str(tmp_path / "rho.cube")
        res.write_cube(path, st, plane=plane)
        lines = open(path).read().split("\n")
        head = [ln.split() for ln in lines[2:6]]
        assert int(head[0][0]) == 2
        n = [int(h[0]) for h in head[1:]]
        vecs = np.array([[float(v) for v in h[1:]] for h in head[1:]])
        assert n == [3, 4, 7] and np.array_equal(vecs, cell / np.array([3.0, 4.0, 7.0])[:, None] / D.BOHR)
        assert np.array_equal(np.array([float(v) for v in head[0][1:]]), 0.5 * vecs.sum(axis=0))
        atoms = [ln.split() for ln in lines[6:8]]
        assert [int(a[0]) for a in atoms] == [3, 8] and np.array_equal(np.array([[float(v) for v in a[2:]] for a in atoms]), st.positions / D.BOHR)
        values = np.array([float(v) for ln in lines[8:] for v in ln.split()])
        src = counts.sum(axis=0) if plane is None else counts[plane]
        exp = src.astype(np.float64) / (10.0 * res.voxel_volume) * D.BOHR ** 3
        assert np.array_equal(values, exp.reshape(-1))
        assert all(len(ln.split()) <= 6 for ln in lines[8:])
    assert abs(res.voxel_volume * 84 - abs(np.linalg.det(cell))) < 1e-12


def test_free_energy_density_and_centers():
    counts = np.zeros((2, 2, 3, 4), dtype=np.uint64)
    counts[0, 1, 2, 3], counts[0, 0, 0, 0], counts[1, 0, 0, 0] = 8, 2, 2
    res = result_of(counts, CUBIC, n_frames=4)
    fe = res.free_energy(0.025)
    assert fe[1, 2, 3] == 0.0 and np.isinf(fe[0, 1, 1]) and fe[0, 0, 0] == pytest.approx(0.025 * np.log(2.0)) and np.isinf(fe).sum() == 22
    fe0 = res.free_energy(0.025, plane=1)
    assert fe0[0, 0, 0] == 0.0 and np.isinf(fe0).sum() == 23
    assert res.voxel_volume == pytest.approx(216.0 / 24) and np.array_equal(res.density, counts / (4.0 * res.voxel_volume))
    fc = res.fractional_centers()
    assert fc.shape == (2, 3, 4, 3) and list(fc[1, 2, 3]) == [0.75, 2.5 / 3, 0.875]
    assert np.allclose(res.cartesian_centers()[1, 0, 0], [4.5, 1.0, 0.75])
    assert np.array_equal(res.voxel_of(res.cartesian_centers().reshape(-1, 3)), np.arange(24))
    empty = result_of(np.zeros((1, 2, 2, 2), dtype=np.uint64), CUBIC).free_energy(0.025)
    assert empty.shape == (2, 2, 2) and np.all(np.isinf(empty)) and np.all(empty > 0)    # nowhere is a maximum
    sm = np.zeros(counts.shape)
    sm[0, 0, 1, 1] = 1.0
    assert result_of(counts, CUBIC, smoothed=sm).free_energy(1.0)[0, 1, 1] == 0.0        # the smoothed grid where there is one


def test_plan_restatement_edges():
    assert R.plan(100, 5, 5, (4, 4, 4))["runs"] == 2 and R.plan(64, 5, 5, (4, 4, 4))["runs"] == 1
    assert R.plan(100, 5, 5, (4, 4, 4), stride=200)["taken"] == 1
    assert R.plan(100, 5, 5, (1025, 4, 4)) is None and R.plan(100, 5, 5, (1024, 1024, 128)) is not None
    assert R.plan(100, 5, 5, (1024, 1024, 128), K=3, n_classes=2) is None
    assert R.slot(0) == 0 and 0 <= R.slot(12345) < R.SLOTS and R.probe(R.SLOTS - 1, 1) == 0
    assert R.halo([[1, -2, 0], [0, 1, 3]], (5, 5, 7)) == [1, 2, 3] and R.halo([[0, 0, 4]], (5, 5, 7)) is None
