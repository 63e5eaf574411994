"""CPU-only: the decisions of the landmark pruning tables (sitator_amd/csrc/candidates_plan.h: periodic distance tests,
bound, box, pair test, critical vertex, grid, covering radius, per-bin sort) compiled with the host compiler under
ASan / UBSan the way test_label_scan.py compiles the label scans.  The probe builds a whole table with cand_build_host
- the serial twin of k_cand_pass / k_cand_scan / k_cand_sort - and tests/candidates_ref.py, an exhaustive periodic
reference in numpy that shares no code with the header, says what that table must contain.

The cases (cases(), CASE_TABLES) reach what no trajectory of the suite does: cells so small that the image search needs two and more
images per axis, a box that covers the whole grid, a skewed cell, a slab with one bin on an axis, a cell so large that
the grid clamps at 192 and is thinned, ragged landmarks, a vertex on a bin-centre plane and a cell face.
tests/test_gpu_candidates.py reads the DEVICE tables of the same cases back and compares them with the probe's."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import candidates_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIDPOINT, STEEPNESS, STATIC_THR = 1.5, 30.0, 1.0
RZ = MIDPOINT + math.log((1 / 0.0001) - 1.) / STEEPNESS       # landmark/helpers.pyx:127-131, as sit_set_basis computes it
LOOSE = (STATIC_THR, 1.0)                                     # (displacement, bin target) of sit_set_basis' table
TIGHT = (0.05, 0.5)                                           # a tight table as ensure_tight_table builds it

# stdin: int64 S D Vp; float64 cm[9] ci[9] rz displacement bin_target; float64 ref[S, 3]; int32 verts[D, Vp];
# float64 vcd[D, Vp].  stdout: int64 G[3] W total; float64 displacement rb h[3]; int32 off[nb + 1]; int32 list[total];
# uint8 crit[total].  Every input array is a heap block of exactly its size: ASan sees a read one element beyond.
PROBE = r"""
#include <stdio.h>
#include <stdlib.h>
#include "candidates_plan.h"

template <class T> static T *take(size_t n)
{
    T *p = (T *)malloc(n * sizeof(T) + (n ? 0 : 1));
    if (n && fread(p, sizeof(T), n, stdin) != n) exit(2);
    return p;
}

int main()
{
    int64_t *head = take<int64_t>(3);
    const int64_t S = head[0], D = head[1], Vp = head[2];
    double *geo = take<double>(21);
    double *ref = take<double>((size_t)(3 * S));
    int32_t *verts = take<int32_t>((size_t)(D * Vp));
    double *vcd = take<double>((size_t)(D * Vp));
    CandArgs a;
    cand_setup(a, geo, geo + 9, geo[19], geo[20]);
    a.ref_static = ref; a.verts = verts; a.vcd = vcd; a.D = D; a.Vp = Vp; a.rz = geo[18];
    CandTable t;
    cand_build_host(a, t);
    const int64_t ints[5] = {a.G[0], a.G[1], a.G[2], t.W, t.total};
    const double reals[5] = {a.displacement, a.rb, a.h[0], a.h[1], a.h[2]};
    fwrite(ints, 8, 5, stdout); fwrite(reals, 8, 5, stdout);
    fwrite(t.off.data(), 4, t.off.size(), stdout);
    fwrite(t.list.data(), 4, t.list.size(), stdout);
    fwrite(t.crit.data(), 1, t.crit.size(), stdout);
    free(head); free(geo); free(ref); free(verts); free(vcd);
    return 0;
}
"""


class Case(object):
    """A cell, reference positions, ragged vertex lists and the centre-vertex distances of the landmarks."""

    def __init__(self, name, cell, static_pos, centers, vertices, tight=False, exact_below=None):
        from oracle import oracle
        self.name = name
        self.cell = np.ascontiguousarray(cell, dtype=np.float64)
        self.ref_static = np.ascontiguousarray(static_pos, dtype=np.float64)
        self.centers = np.ascontiguousarray(centers, dtype=np.float64)
        self.vertices = [list(v) for v in vertices]
        self.tables = [LOOSE, TIGHT] if tight else [LOOSE]
        self.exact_below = exact_below
        self.S, self.D = len(self.ref_static), len(self.vertices)
        self.V = max(1, max(len(v) for v in self.vertices))
        self.Vp = (self.V + 3) // 4 * 4
        self.verts = np.full((self.D, self.V), -1, dtype=np.int64)           # what sit_set_basis is given
        self.vcd = np.full((self.D, self.V), np.nan)
        for k, v in enumerate(self.vertices):
            self.verts[k, :len(v)] = v
            if len(v):
                self.vcd[k, :len(v)] = oracle.distances(self.cell, self.centers[k], self.ref_static[v])
        self.verts_p = np.full((self.D, self.Vp), -1, dtype=np.int32)        # what it uploads: -1 / 1.0 padded to Vp
        self.vcd_p = np.ones((self.D, self.Vp))
        self.verts_p[:, :self.V] = self.verts
        self.vcd_p[:, :self.V] = np.where(self.verts >= 0, self.vcd, 1.0)
        self._refs = {}

    def reference(self, displacement, G):
        key = (float(displacement), tuple(int(g) for g in G))
        if key not in self._refs:
            self._refs[key] = R.Reference(self.cell, self.ref_static, self.verts_p, self.vcd_p, RZ, displacement, G, self.exact_below)
        return self._refs[key]

    def probe_input(self, displacement, bin_target):
        cm = np.ascontiguousarray(self.cell.T)
        ci = np.ascontiguousarray(np.linalg.inv(self.cell.T))                # as HipContext hands it to sit_create
        return b"".join([np.array([self.S, self.D, self.Vp], dtype=np.int64).tobytes(), cm.tobytes(), ci.tobytes(),
                         np.array([RZ, displacement, bin_target]).tobytes(), self.ref_static.tobytes(),
                         np.ascontiguousarray(self.verts_p).tobytes(), np.ascontiguousarray(self.vcd_p).tobytes()])


def _sc_grid(G, cell):
    """synth.sc_grid without its lower limit of three cells per axis."""
    g = np.array([(a, b, c) for a in range(G[0]) for b in range(G[1]) for c in range(G[2])])
    Gf = np.asarray(G, dtype=np.float64)
    sidx = lambda a, b, c: ((a % G[0]) * G[1] + (b % G[1])) * G[2] + (c % G[2])
    vertices = [[int(sidx(a + dx, b + dy, c + dz)) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)] for a, b, c in g]
    return ((g + 0.25) / Gf) @ cell, ((g + 0.75) / Gf) @ cell, vertices


def _scattered(cell, n_static, n_landmarks, seed, far=0.5):
    """Static atoms at seeded fractional positions; landmarks at seeded centres whose four vertices are the nearest
    atoms or (a share of `far`) four atoms drawn at random, so that some centre-vertex distances are long."""
    from sitator_amd import synth
    rng = np.random.default_rng(seed)
    static = rng.random((n_static, 3)) @ cell
    centers = rng.random((n_landmarks, 3)) @ cell
    vertices = []
    for k, c in enumerate(centers):
        d = synth.mic_displacement(static - c, cell)
        order = np.argsort(np.einsum("ij,ij->i", d, d), kind="stable")
        vertices.append([int(x) for x in (rng.permutation(n_static)[:4] if rng.random() < far else order[:4])])
    return static, centers, vertices


def _make_cases():
    from sitator_amd import synth
    out = []
    h = synth.config_host("C1d")
    out.append(Case("ortho_c1d", h.cell, h.static_pos, h.centers, h.vertices, tight=True))
    cell = np.diag([8.0, 8.8, 9.6])
    # (its loose table lists all 8 landmarks in all 720 bins: that one exercises the whole-grid branch of the box and the
    # images an atom is its own neighbour through, not the bound - only the tight table leaves anything out)
    out.append(Case("ortho_2x2x2", cell, *_sc_grid((2, 2, 2), cell), tight=True))
    cell = synth.hexagonal_cell(7.0, 6.5)
    out.append(Case("hexagonal_7", cell, *_scattered(cell, 10, 14, seed=7), tight=True))
    cell = np.array([[9.0, 0, 0], [7.5, 5.0, 0], [6.0, 3.5, 3.8]])
    out.append(Case("triclinic_skewed", cell, *_scattered(cell, 10, 14, seed=8), tight=True))
    cell = np.diag([10.0, 1.4, 10.5])
    out.append(Case("slab_1p4", cell, *_scattered(cell, 6, 8, seed=9)))
    # four landmarks of four vertices: one around the cell's corner (its vertices wrap on all three axes), one across the
    # x = 0 face, one across the z face, one inside; bins of the lists wrap through index 0
    cell = np.diag([400.0, 300.0, 100.0])
    static = np.array([[1.2, 1.0, 0.8], [398.9, 1.1, 99.4], [1.0, 298.8, 99.5], [399.0, 299.1, 0.9],
                       [1.5, 150.0, 50.0], [398.5, 151.5, 50.5], [399.5, 149.0, 51.5], [0.7, 151.0, 48.5],
                       [200.0, 100.0, 99.3], [201.0, 101.5, 0.6], [199.0, 101.0, 0.9], [200.5, 99.0, 98.9],
                       [120.0, 80.0, 40.0], [122.0, 81.0, 41.0], [121.0, 82.5, 39.0], [119.5, 81.0, 41.5]])
    centers = np.array([[0.0, 0.0, 0.1], [0.0, 150.4, 50.1], [200.1, 100.4, 0.0], [120.6, 81.1, 40.4]])
    out.append(Case("large_400x300x100", cell, static, centers, [list(range(4 * k, 4 * k + 4)) for k in range(4)],
                    exact_below="auto"))
    # ragged: 1, 4, 6 and 8 vertices, atom 0 in most landmarks, landmarks 3 and 4 with identical vertex sets; and the same with a
    # landmark without any vertex, which sit_set_basis and the oracle both accept: the oracle's component for it is 1.0
    # wherever the ion is (test_a_landmark_without_vertices_is_listed_everywhere asks it), so every bin must list it
    cell = np.diag([9.0, 10.0, 11.0])
    rng = np.random.default_rng(10)
    static = rng.random((12, 3)) @ cell
    centers = rng.random((9, 3)) @ cell
    vertices = [[0], [0, 1, 2, 3], [0, 4, 5, 6, 7, 8], [0, 2, 5, 9], [0, 2, 5, 9], [0, 1, 2, 3, 4, 5, 6, 7], [10],
                [0, 3, 6, 9, 10, 11], [11, 0, 1, 4]]
    out.append(Case("ragged", cell, static, centers, vertices, tight=True))
    out.append(Case("ragged_with_empty", cell, static, np.concatenate([centers, [[1.0, 2.0, 3.0]]]), vertices + [[]], tight=True))
    # (What the +-1e-9 in the box's ceil / floor decide is only whether a bin whose centre is EXACTLY the tightest bound
    # away along an axis is walked; the pair test then meets the same bound, so such a pair lies on the lower edge of the
    # undecided band whatever the box does, and a case tuned onto it would have nothing to assert.)
    # landmark 0 has one vertex, atom 0, on the cell faces x = 0 and z = 0 and on the bin-centre plane y = 3.5 / 11;
    # landmark 1's tightest vertex is atom 1 on x = 4.5 / 10 (a bin-centre plane), y = 0, z = 11.5 / 12
    cell = np.diag([10.0, 11.0, 12.0])
    static = np.array([[0.0, 3.5 / 11, 0.0], [4.5 / 10, 0.0, 11.5 / 12], [0.31, 0.07, 0.9], [0.52, 0.13, 0.83],
                       [0.4, 0.93, 0.05]]) @ cell
    centers = np.array([static[0] + [0.9, 0.4, -0.7], static[1] + [0.5, 0.3, 0.2]])
    out.append(Case("on_planes", cell, static, centers, [[0], [1, 2, 3, 4]], tight=True))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in _make_cases()}
    return _CASES


CASE_TABLES = [("ortho_c1d", 0), ("ortho_c1d", 1), ("ortho_2x2x2", 0), ("ortho_2x2x2", 1), ("hexagonal_7", 0),
               ("hexagonal_7", 1), ("triclinic_skewed", 0), ("triclinic_skewed", 1), ("slab_1p4", 0),
               ("large_400x300x100", 0), ("ragged", 0), ("ragged", 1), ("ragged_with_empty", 0), ("ragged_with_empty", 1), ("on_planes", 0),
               ("on_planes", 1)]


def build_probe(directory, header_dir=None):
    """Compiles the probe (ASan + UBSan, no contraction) against candidates_plan.h of `header_dir`; returns run(case,
    displacement, bin_target) -> (table dict, W, h[3])."""
    src = os.path.join(str(directory), "probe.cpp")
    with open(src, "w") as f:
        f.write(PROBE)
    exe = os.path.join(str(directory), "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", header_dir or os.path.join(ROOT, "sitator_amd", "csrc"), src,
                           "-o", exe])

    def run(case, displacement, bin_target):
        out = subprocess.run([exe], input=case.probe_input(displacement, bin_target), stdout=subprocess.PIPE, check=True).stdout
        ints = np.frombuffer(out, dtype=np.int64, count=5)
        reals = np.frombuffer(out, dtype=np.float64, count=5, offset=40)
        nb, total = int(ints[0] * ints[1] * ints[2]), int(ints[4])
        off = np.frombuffer(out, dtype=np.int32, count=nb + 1, offset=80)
        lst = np.frombuffer(out, dtype=np.int32, count=total, offset=80 + 4 * (nb + 1))
        crit = np.frombuffer(out, dtype=np.uint8, count=total, offset=80 + 4 * (nb + 1) + 4 * total)
        assert len(out) == 80 + 4 * (nb + 1) + 5 * total
        table = {"grid": [int(x) for x in ints[:3]], "displacement": float(reals[0]), "rb": float(reals[1]), "total": total,
                 "off": off, "list": lst, "crit": crit}
        return table, int(ints[3]), reals[2:5].copy()
    return run


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build_probe(tmp_path_factory.mktemp("candidates_plan"))


@pytest.mark.parametrize("name,which", CASE_TABLES)
def test_host_table_against_the_exhaustive_reference(probe, name, which):
    """cand_build_host's table is complete (every pair with margin >= 0 listed), lists nothing beyond the code's pads,
    is well formed, names critical vertices with the least room and reports the grid of the reference formula; fewer
    than 0.1 % of its pairs sit inside the pads, where either answer is right.  (The probe reports no mean: that one is
    compared on the device, tests/test_gpu_candidates.py.)"""
    case = cases()[name]
    displacement, bin_target = case.tables[which]
    table, W, h = probe(case, displacement, bin_target)
    assert table["grid"] == R.grid_of(case.cell, bin_target)
    assert table["displacement"] == displacement
    np.testing.assert_allclose(h, R.heights(case.cell), rtol=1e-12)
    ref = case.reference(displacement, table["grid"])
    assert abs(table["rb"] - (ref.rb_true + 1e-6)) < 1e-12
    total, undecided, share = R.check_table(ref, table, W=W, label="%s/%d" % (name, which))
    print("%s table %d: grid %s, %d pairs listed, %d undecided (%.4f %%), images per axis %s" % (
        name, which, table["grid"], total, undecided, 100 * share, list(ref.images_per_axis())))
    assert total > 0


def test_a_landmark_without_vertices_is_listed_everywhere(probe):
    """The oracle decides: with the ion on every bin centre of the loose grid, the component of the landmark without
    vertices is 1.0 - so its list is every bin, and the host table has it there (critical vertex 0)."""
    from oracle import oracle
    case = cases()["ragged_with_empty"]
    k = case.D - 1
    assert case.vertices[k] == [] and (case.verts[k] == -1).all()
    table, _, _ = probe(case, *LOOSE)
    centres = R.bin_centres(case.cell, table["grid"])
    frames = np.repeat(np.concatenate([case.ref_static, [[0.0, 0.0, 0.0]]])[None], len(centres), axis=0)
    frames[:, -1] = centres
    rows, _ = oracle.fill(case.cell, oracle.wrap_points(case.cell, frames), np.arange(case.S), np.array([case.S]), case.ref_static,
                          case.verts, case.vcd, MIDPOINT, STEEPNESS, STATIC_THR, check_for_zeros=False)
    assert (rows[:, k] == 1.0).all()
    holds = np.zeros(len(centres), dtype=bool)
    sel = table["list"] == k
    holds[np.repeat(np.arange(len(centres)), np.diff(table["off"]))[sel]] = True
    assert holds.all() and (table["crit"][sel] == 0).all()


def test_the_cases_reach_the_regimes_they_are_named_for(probe):
    """Asserted from the cases themselves: which branch of the image search, the box and the grid each one takes."""
    c = cases()
    n = lambda name: c[name].reference(STATIC_THR, R.grid_of(c[name].cell, 1.0)).images_per_axis()
    assert list(n("ortho_c1d")) == [1, 1, 1]
    assert n("hexagonal_7").max() >= 2 and n("triclinic_skewed").max() >= 2 and n("slab_1p4").max() >= 4
    assert R.heights(c["triclinic_skewed"].cell).min() <= 4.0 and np.linalg.norm(c["triclinic_skewed"].cell, axis=1).min() > 7.5
    assert R.grid_of(c["slab_1p4"].cell, 1.0)[1] == 1
    # the large cell: clamped at 192 on two axes, then thinned; about 1.2e6 bins; lists on both sides of bin index 0
    G = R.grid_of(c["large_400x300x100"].cell, 1.0)
    assert G == [108, 108, 100] and max(G) < 192 < 300 and 1.1e6 < G[0] * G[1] * G[2] <= 1.5e6
    table, _, _ = probe(c["large_400x300x100"], *LOOSE)
    length = np.diff(table["off"])
    assert length[0] > 0 and length[-1] > 0 and (length == 0).sum() > 1000000
    # the 2 x 2 x 2 host: every landmark's box is the whole grid (all bins hold all landmarks or the test says which)
    table, _, _ = probe(c["ortho_2x2x2"], *LOOSE)
    ref = c["ortho_2x2x2"].reference(STATIC_THR, table["grid"])
    assert (2 * ref.T_max / R.heights(c["ortho_2x2x2"].cell) >= 1.0).all()
    # the same reference with and without skipping the pairs that are certainly out of reach
    small = c["hexagonal_7"]
    a = small.reference(STATIC_THR, R.grid_of(small.cell, 1.0))
    b = R.Reference(small.cell, small.ref_static, small.verts_p, small.vcd_p, RZ, STATIC_THR, a.G, "auto")
    near = a.margin > -0.5
    assert np.array_equal(near, b.margin > -0.5) and np.array_equal(a.margin[near], b.margin[near])


# ---- frames at the edge the bound exists for (shared with tests/test_gpu_candidates.py) ---------------------------------

EDGE_CELLS = ["ortho_c1d", "hexagonal_7", "triclinic_skewed"]
_EDGE = {}


def _towards(cell, a, b, N):
    """The shortest of the vectors from a to the images of b in [-N, N]^3 of the round-reduced difference."""
    f = (b - a) @ np.linalg.inv(cell)
    f -= np.round(f)
    rng = np.arange(-N, N + 1)
    img = np.array([(i, j, k) for i in rng for j in rng for k in rng], dtype=np.float64)
    r = (f[None, :] + img) @ cell
    return r[np.argmin(np.einsum("ij,ij->i", r, r))]


def neighbours(q):
    """q and, per coordinate, q moved by -8, -1, +1, +8 ulps (tests/test_gpu_boundaries.py's _neighbours)."""
    out = [np.array(q, dtype=np.float64)]
    for axis in range(3):
        for n in (-8, -1, 1, 8):
            p = np.array(q, dtype=np.float64)
            for _ in range(abs(n)):
                p[axis] = np.nextafter(p[axis], np.inf if n > 0 else -np.inf)
            out.append(p)
    return out


def edge_frames(name, n_landmarks=12, per_landmark=8):
    """One mobile ion on corners q of the loose grid, the vertex atoms of one landmark k moved straight towards q by
    (1 - 1e-6) static_thr, every other atom on its reference position; then the ulp neighbours of q.  Per landmark the
    corners are those within reach of k (k can still be non-zero there) next to the bins the table lists most narrowly.  Returns (frames [n, S + 1, 3], oracle rows
    [n, D], n_all_zero): the oracle accepts every frame."""
    from oracle import oracle
    if name in _EDGE:
        return _EDGE[name]
    case = cases()[name]
    cell, ref_static = case.cell, case.ref_static
    G = R.grid_of(cell, LOOSE[1])
    ix, iy, iz = np.meshgrid(np.arange(G[0]), np.arange(G[1]), np.arange(G[2]), indexing="ij")
    corners = (np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) / np.asarray(G, dtype=np.float64)) @ cell
    move = (1.0 - 1e-6) * STATIC_THR
    T = float(RZ * np.nanmax(case.vcd) + STATIC_THR)
    N = int(np.ceil(T / R.heights(cell).min())) + 1
    rng = np.random.default_rng(3)
    margin = case.reference(STATIC_THR, G).margin
    frames = []
    for k in rng.permutation(case.D)[:n_landmarks]:
        v = case.vertices[k]
        spare = np.min([RZ * case.vcd[k, h] + move - R.periodic_distance(cell, corners, ref_static[s], T) for h, s in enumerate(v)], axis=0)
        # ... and, among those, the corners one of whose eight bins has the smallest reference margin for k
        Mk = margin[:, k].reshape(G)
        tightest = np.min([np.roll(Mk, (a, b, c), axis=(0, 1, 2)) for a in (0, 1) for b in (0, 1) for c in (0, 1)], axis=0).ravel()
        order = np.argsort(np.where(spare > 1e-3, tightest, np.inf), kind="stable")
        for c in order[:per_landmark]:
            if not spare[c] > 1e-3:
                break
            q = corners[c]
            fr = np.concatenate([ref_static, [q]])
            for s in set(v):
                d = _towards(cell, ref_static[s], q, N)
                fr[s] = ref_static[s] + d / np.linalg.norm(d) * move
                moved = float(oracle.distances(cell, ref_static[s], fr[s][None])[0])
                assert (1.0 - 3e-6) * STATIC_THR < moved <= STATIC_THR, (name, k, s, moved)
            for p in neighbours(q):
                one = fr.copy()
                one[-1] = p
                frames.append(one)
    frames = np.array(frames)
    S = case.S
    rows, nz = oracle.fill(cell, oracle.wrap_points(cell, frames), np.arange(S), np.array([S]), ref_static, case.verts, case.vcd,
                           MIDPOINT, STEEPNESS, STATIC_THR, check_for_zeros=False)
    _EDGE[name] = (frames, rows, nz)
    return _EDGE[name]


def edge_reach(name, frames, rows):
    """(pairs near the bound, pairs far from the bin centre): distinct (ion bin, landmark) pairs with a non-zero oracle
    component whose reference margin in the loose table is below static_thr / 2 - a table built without the displacement
    term drops them - and those whose ion is further than rb_true / 2 from the centre of its bin."""
    case = cases()[name]
    ref = case.reference(STATIC_THR, R.grid_of(case.cell, LOOSE[1]))
    G = np.asarray(ref.G)
    frac = frames[:, -1] @ np.linalg.inv(case.cell)
    frac -= np.floor(frac)
    b3 = np.floor(frac * G).astype(np.int64) % G
    bins = (b3[:, 0] * G[1] + b3[:, 1]) * G[2] + b3[:, 2]
    off_centre = np.array([R.periodic_distance(case.cell, frames[i:i + 1, -1], ref.centres[b], ref.rb_true + 1.0)[0]
                           for i, b in enumerate(bins)])
    f, k = np.nonzero(rows)
    m = ref.margin[bins[f], k]
    assert (m >= 0).all(), "a non-zero component outside the reference's bound: the bound's derivation is wrong"
    near = set(zip(bins[f][m < STATIC_THR / 2], k[m < STATIC_THR / 2]))
    far_sel = off_centre[f] > ref.rb_true / 2
    far = set(zip(bins[f][far_sel], k[far_sel]))
    return len(near), len(far)


@pytest.mark.parametrize("name", EDGE_CELLS)
def test_edge_frames_reach_the_edge(probe, name):
    """The frames of the GPU row test are where they claim to be: at least 20 non-zero (ion bin, landmark) pairs with a
    reference margin below static_thr / 2 and at least 20 with the ion beyond rb_true / 2 from its bin's centre - and the
    host table lists every pair the oracle found non-zero (with the neighbouring bins of an ion on a corner)."""
    frames, rows, nz = edge_frames(name)
    near, far = edge_reach(name, frames, rows)
    print("%s: %d frames, %d non-zero components, %d pairs near the bound, %d far from the bin centre" % (
        name, len(frames), int((rows != 0).sum()), near, far))
    assert near >= 20 and far >= 20
    case = cases()[name]
    table, _, _ = probe(case, *LOOSE)
    G = np.asarray(table["grid"])
    listed = np.zeros((int(G.prod()), case.D), dtype=bool)
    listed[np.repeat(np.arange(len(listed)), np.diff(table["off"])), table["list"]] = True
    frac = frames[:, -1] @ np.linalg.inv(case.cell)
    frac -= np.floor(frac)
    b3 = np.floor(frac * G).astype(np.int64) % G
    f, k = np.nonzero(rows)
    assert listed[(b3[f, 0] * G[1] + b3[f, 1]) * G[2] + b3[f, 2], k].all()
