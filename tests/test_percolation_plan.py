"""CPU-only: the decisions of DensityPercolation (sitator_amd/csrc/percolation_plan.h) compiled with the host compiler under ASan /
UBSan into a stand-alone probe, the way test_density_plan.py builds its own, and driven over stdin / stdout; tests/percolation_ref.py
says what must come out.  Everything is an integer or the bytes of a double: no tolerance."""
import os
import subprocess

import numpy as np
import pytest

from tests import percolation_ref as R
from tests.test_percolation_ref import S, saddle_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: int64 mode, N, K.
#   mode 0: (N = n of an axis)                               -> int64 [N][3][2]: pc_neighbour(i, d) for d = -1, 0, 1: (j, s)
#   mode 1: int64 n[3] (K = connectivity)                    -> int64 [V][27][5]: neighbour, code, offset in the connectivity, interior forward,
#           seam forward
#   mode 2: int64 n[3]; float64 level; float64 grid[N] (K = 100 * tile_first + connectivity)
#           -> int64 ok, rounds, seam records, distinct, cycles, n_pairs, n_comps; int64 label[N]; int64 comps[n_comps][11]
#   mode 3: int64 v[N][3]                                    -> int64 ok, rank; 9 x 16 bytes: the rows as little-endian 128-bit integers;
#           int64 fits, basis[9] (pc_lattice_basis)
#   mode 4: (K = lo_bits as int64) float64 g[N]              -> int64 candidate[N]; int64 above, top, below (pc_range_serial)
#   mode 5: int64 n[3]; float64 grid[N] (K as mode 2)        -> int64 ok, passes, ranks[3]; float64 levels[3] (as 8 bytes each)
#   mode 6: int64 n[3], connectivity, form, cap              -> int64 err, V, n_tiles, lds_bytes, seam_max, form, blocks, workspace, layout
#           layout: pc_layout() on a null base and on a made-up one - 0, or the sum of 1 (the two runs disagree or the levels' buffer is
#           not the plan's workspace), 2 (a piece is not 256-byte aligned), 4 (two pieces overlap, or one ends beyond the buffer)
#   mode 7: int64 rec[N][3] (K = first_full_ends)            -> int64 ok, max_rank, cycles, distinct, n_pairs, n_comps; pairs; comps[..][11]
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "percolation_plan.h"

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }
static void wr1(int64_t v) { wr(&v, 8, 1); }

static void wr_quotient(const PcQuotient &q)
{
    for (size_t i = 0; i < q.pairs.size(); i++) wr1(q.pairs[i]);
    for (size_t i = 0; i < q.comps.size(); i++) {
        wr1(q.comps[i].root); wr1(q.comps[i].rank);
        for (int k = 0; k < 9; k++) wr1(q.comps[i].basis[k]);
    }
}

static int layout_of(const PcPlan &p, int64_t cap)
{
    Carve sized = {nullptr, 0}, cv = {(char *)((uintptr_t)1 << 40), 0}, lv = {nullptr, 0};
    pc_layout(sized, p, cap);
    pc_layout(lv, p, -1);
    const PcPieces w = pc_layout(cv, p, cap);
    struct Piece { const void *at; int64_t bytes; };
    const Piece pieces[] = {{w.grid, p.V * 8}, {w.label, p.V * 4}, {w.words, PC_WORDS * 8}, {w.seam, p.seam_max * 12},
                            {w.size, cap < 0 ? 0 : p.V * 4}, {w.block_count, cap < 0 ? 0 : p.blocks * 4},
                            {w.offsets, cap < 0 ? 0 : (p.blocks + 1) * 8}, {w.out, cap < 0 ? 0 : cap * 16}};
    int bad = 0;
    if (sized.used != cv.used || lv.used != p.workspace || w.head != p.workspace || (cap < 0 && cv.used != p.workspace)) bad |= 1;
    int64_t end = 0;
    for (int i = 0; i < 8; i++) {
        const int64_t off = (int64_t)((uintptr_t)pieces[i].at - (uintptr_t)cv.base);
        if (off % 256) bad |= 2;
        if (off < end) bad |= 4;
        end = off + pieces[i].bytes;
    }
    if (end > cv.used) bad |= 4;
    return bad;
}

int main()
{
    int64_t h[3];
    if (fread(h, 8, 3, stdin) != 3) return 2;
    const int64_t mode = h[0], N = h[1], K = h[2];
    if (N < 0 || N > 10000000) return 3;
    const size_t n = (size_t)N;
    if (mode == 0) {
        for (int64_t i = 0; i < N; i++)
            for (int d = -1; d <= 1; d++) {
                int64_t j; int s;
                pc_neighbour(i, d, N, &j, &s);
                wr1(j); wr1(s);
            }
        return 0;
    }
    if (mode == 1) {
        int64_t g[3];
        if (!rd(g, 8, 3)) return 2;
        const int64_t V = g[0] * g[1] * g[2];
        for (int64_t v = 0; v < V; v++) {
            int64_t i[3];
            pc_coords(v, g, i);
            for (int k = 0; k < 27; k++) {
                int code;
                const int64_t u = pc_edge(i, g, k, &code);
                wr1(u); wr1(code); wr1(k != PC_NO_OFFSET && pc_offset_in((int)K, k)); wr1(pc_is_interior_forward(k, code)); wr1(pc_is_seam_forward(code));
            }
        }
        return 0;
    }
    if (mode == 2 || mode == 5) {
        int64_t g[3]; double level = 0;
        if (!rd(g, 8, 3) || (mode == 2 && !rd(&level, 8, 1))) return 2;
        if (g[0] < 1 || g[1] < 1 || g[2] < 1 || g[0] * g[1] * g[2] != N) return 3;
        std::vector<double> grid(n);
        if (!rd(grid.data(), 8, n)) return 2;
        const int conn = (int)(K % 100); const bool tile_first = K >= 100;
        if (mode == 5) {
            double levels[3]; int32_t ranks[3]; int64_t passes;
            const bool ok = pc_levels_serial(grid.data(), g, conn, tile_first, levels, ranks, &passes);
            wr1(ok); wr1(passes);
            for (int d = 0; d < 3; d++) wr1(ranks[d]);
            wr(levels, 8, 3);
            return 0;
        }
        std::vector<int32_t> label(n);
        PcQuotient q;
        int64_t rounds, n_rec;
        const bool ok = pc_components_serial(grid.data(), g, level, conn, tile_first, label.data(), q, &rounds, &n_rec);
        wr1(ok); wr1(rounds); wr1(n_rec); wr1(q.distinct); wr1(q.cycles); wr1((int64_t)q.pairs.size() / 2); wr1((int64_t)q.comps.size());
        for (size_t v = 0; v < n; v++) wr1(label[v]);
        for (size_t i = 0; i < q.comps.size(); i++) {
            wr1(q.comps[i].root); wr1(q.comps[i].rank);
            for (int k = 0; k < 9; k++) wr1(q.comps[i].basis[k]);
        }
        return 0;
    }
    if (mode == 3) {
        std::vector<int64_t> v(3 * n);
        if (!rd(v.data(), 8, 3 * n)) return 2;
        PcLattice L;
        pc_lattice_clear(L);
        bool ok = true;
        for (size_t i = 0; i < n && ok; i++) {
            const pc_wide w[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
            ok = pc_hnf_insert(L, w);
        }
        pc_wide rows[3][3];
        pc_lattice_rows(L, rows);
        int32_t basis[9] = {0};
        const bool fits = pc_lattice_basis(L, basis);
        wr1(ok); wr1(L.rank);
        wr(rows, 16, 9);
        wr1(fits);
        for (int k = 0; k < 9; k++) wr1(basis[k]);
        return 0;
    }
    if (mode == 4) {
        std::vector<double> g(n);
        if (!rd(g.data(), 8, n)) return 2;
        for (size_t i = 0; i < n; i++) wr1(pc_candidate(g[i], (uint64_t)K));
        uint64_t above, top, below;
        pc_range_serial(g.data(), N, (uint64_t)K, &above, &top, &below);
        wr(&above, 8, 1); wr(&top, 8, 1); wr(&below, 8, 1);
        return 0;
    }
    if (mode == 6) {
        int64_t a[6];
        if (!rd(a, 8, 6)) return 2;
        const PcPlan p = pc_plan(a, (int)a[3], (int)a[4]);
        wr1(p.err ? 1 : 0); wr1(p.V); wr1(p.n_tiles); wr1(p.lds_bytes); wr1(p.seam_max); wr1(p.form); wr1(p.blocks); wr1(p.workspace);
        wr1(p.err ? 0 : layout_of(p, a[5]));
        return 0;
    }
    if (mode == 7) {
        std::vector<int32_t> rec(3 * n);
        std::vector<int64_t> in(3 * n);
        if (!rd(in.data(), 8, 3 * n)) return 2;
        for (size_t i = 0; i < 3 * n; i++) rec[i] = (int32_t)in[i];
        PcQuotient q;
        const bool ok = pc_quotient(rec.data(), N, K != 0, q);
        wr1(ok); wr1(q.max_rank); wr1(q.cycles); wr1(q.distinct); wr1((int64_t)q.pairs.size() / 2); wr1((int64_t)q.comps.size());
        wr_quotient(q);
        return 0;
    }
    return 3;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("percolation_plan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])

    def run(mode, N, K, *arrays, raw=False):
        data = np.array([mode, N, K], dtype=np.int64).tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
        out = subprocess.run([exe], input=data, stdout=subprocess.PIPE, check=True).stdout
        return out if raw else np.frombuffer(out, dtype=np.int64)
    return run


@pytest.mark.parametrize("n", [1, 2, 3, 1024])
def test_neighbour_and_shift_on_every_offset(probe, n):
    got = probe(0, n, 0).reshape(n, 3, 2)
    for i in (range(n) if n <= 3 else (0, 1, 511, 1022, 1023)):
        for k, d in enumerate((-1, 0, 1)):
            j, s = R.neighbour((i, 0, 0), (d, 0, 0), (n, 1, 1))
            assert (got[i, k, 0], got[i, k, 1]) == (j[0], s[0])
    i = np.arange(n)
    for k, d in enumerate((-1, 0, 1)):
        assert np.array_equal(got[:, k, 0], (i + d) % n) and np.array_equal(got[:, k, 1], (i + d) // n)
    assert got[:, :, 1].min() >= -1 and got[:, :, 1].max() <= 1 and got[:, :, 0].min() >= 0 and got[:, :, 0].max() < n


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("n", [(1, 1, 1), (1, 2, 3), (2, 2, 2), (3, 1, 2), (4, 3, 5)])
def test_edges_of_a_voxel_and_who_looks_at_them(probe, n, connectivity):
    V = n[0] * n[1] * n[2]
    got = probe(1, 0, connectivity, np.array(n, dtype=np.int64)).reshape(V, 27, 5)
    offs = set(R.offsets(connectivity))
    interior, seam = {}, {}
    for v in range(V):
        i = np.unravel_index(v, n)
        for k in range(27):
            d = (k // 9 - 1, k // 3 % 3 - 1, k % 3 - 1)
            j, s = R.neighbour(i, d, n)
            u, code, inside, fwd, sfwd = got[v, k]
            assert u == np.ravel_multi_index(j, n) and code == 9 * (s[0] + 1) + 3 * (s[1] + 1) + s[2] + 1 and bool(inside) == (d in offs)
            assert bool(fwd) == (d > (0, 0, 0) and s == (0, 0, 0)) and bool(sfwd) == (s > (0, 0, 0))
            if d in offs and d != (0, 0, 0):
                if s == (0, 0, 0):
                    interior.setdefault((min(v, u), max(v, u), d if v <= u and d > (0, 0, 0) else tuple(-x for x in d)), []).append(bool(fwd))
                else:
                    key = (v, u, s) if s > (0, 0, 0) else (u, v, tuple(-x for x in s))
                    seam.setdefault(key + (d if s > (0, 0, 0) else tuple(-x for x in d),), []).append(bool(sfwd))
    # every undirected edge is seen from both ends and looked at from exactly one
    assert all(sorted(v) == [False, True] for v in interior.values()) and all(sorted(v) == [False, True] for v in seam.values())
    assert len(seam) == R.seam_max(n, connectivity)


def components(probe, grid, level, connectivity, tile_first=False):
    g = np.ascontiguousarray(grid, dtype=np.float64)
    out = probe(2, g.size, 100 * int(tile_first) + connectivity, np.array(g.shape, dtype=np.int64), np.array([level]), g)
    ok, rounds, n_rec, distinct, cycles, n_pairs, n_comps = (int(v) for v in out[:7])
    assert ok == 1 and rounds >= 1 and distinct <= n_rec <= R.seam_max(g.shape, connectivity)
    labels = out[7:7 + g.size].astype(np.int32).reshape(g.shape)
    comps = out[7 + g.size:].reshape(n_comps, 11)
    return labels, comps, rounds


def check_against_restatement(probe, grid, level, connectivity):
    exp_labels, roots, sizes, rank, basis = R.components(grid, level, connectivity)
    rounds = []
    for tile_first in (False, True):
        labels, comps, r = components(probe, grid, level, connectivity, tile_first)
        rounds.append(r)
        assert np.array_equal(labels, exp_labels)
        with_loops = rank > 0
        assert np.array_equal(comps[:, 0], roots[with_loops]) and np.array_equal(comps[:, 1], rank[with_loops])
        assert np.array_equal(comps[:, 2:].reshape(-1, 3, 3), basis[with_loops])
    return rounds


@pytest.mark.parametrize("case", R.designed(), ids=[c[0] for c in R.designed()])
def test_hook_compress_and_quotient_on_the_designed_grids(probe, case):
    _, grid, level, connectivity, _ = case
    check_against_restatement(probe, grid, level, connectivity)


def test_designed_grids_across_tile_faces(probe):
    """The double loop and the winding channel in a grid of more than one tile along every axis."""
    g = np.zeros((16, 10, 20))
    for i in range(16):
        g[i, (i // 2) % 10, (3 * i) % 20] = 1.0
        g[i, (i // 2 + 1) % 10, (3 * i + 1) % 20] = 1.0
    g[:, 9, 15:18] = 1.0
    for connectivity in (6, 18, 26):
        check_against_restatement(probe, g, 0.5, connectivity)


def test_200_random_grids_of_at_most_512_voxels(probe):
    rng = np.random.default_rng(24)
    seen_ranks = set()
    for trial in range(200):
        shape = tuple(int(v) for v in rng.integers(1, 9, size=3))
        g = rng.random(shape)
        if trial % 7 == 0:
            g.reshape(-1)[rng.integers(0, g.size)] = np.nan
        connectivity = (6, 18, 26)[trial % 3]
        level = float(rng.choice([0.25, 0.5, 0.7, 0.85]))
        check_against_restatement(probe, g, level, connectivity)
        seen_ranks.update(R.components(g, level, connectivity)[3].tolist())
    assert seen_ranks == {0, 1, 2, 3}


def test_serpentine_needs_many_rounds_and_still_settles(probe):
    n = (5, 4, 6)
    g = np.zeros(n)
    path = []
    for i in range(n[0]):
        for jj in range(n[1]):
            j = jj if i % 2 == 0 else n[1] - 1 - jj
            ks = range(n[2]) if (i * n[1] + jj) % 2 == 0 else range(n[2] - 1, -1, -1)
            path.extend((i, j, k) for k in ks)
    assert len(set(path)) == g.size
    for step, v in enumerate(path):
        g[v] = 1.0 + step
    rounds = check_against_restatement(probe, g, 1.0, 6)
    assert rounds[0] >= 1


def hnf_of(probe, vectors):
    v = np.array(vectors, dtype=np.int64).reshape(-1, 3)
    raw = probe(3, len(v), 0, v, raw=True)
    ok, rank = np.frombuffer(raw[:16], dtype=np.int64)
    rows = [int.from_bytes(raw[16 + 16 * k:32 + 16 * k], "little", signed=True) for k in range(9)]
    tail = np.frombuffer(raw[16 + 144:], dtype=np.int64)
    return int(ok), int(rank), [rows[0:3], rows[3:6], rows[6:9]], int(tail[0]), tail[1:].reshape(3, 3).tolist()


def test_hermite_normal_form_on_random_vectors_up_to_2_31(probe):
    rng = np.random.default_rng(31)
    big = 1 << 31
    for trial in range(360):
        kind = trial % 6
        if kind == 0:                                               # any vectors with entries up to 2^31: rank 3 as a rule, whose row Euclid
            vectors = rng.integers(-big, big + 1, size=(int(rng.integers(3, 7)), 3))       # leaves 127 bits before it cancels
        elif kind == 1:                                             # multiples of one small vector
            vectors = rng.integers(-3, 4, size=(1, 3)) * rng.integers(-(big // 3), big // 3 + 1, size=(5, 1))
        elif kind == 2:                                             # large combinations of two small vectors
            vectors = rng.integers(-(1 << 28), 1 << 28, size=(6, 2)) @ rng.integers(-3, 4, size=(2, 3))
        elif kind == 3:                                             # one or two vectors of any kind: rank 2 at most
            vectors = rng.integers(-big, big + 1, size=(int(rng.integers(1, 3)), 3))
        elif kind == 4:                                             # shift sums as the quotient meets them, and some more
            vectors = rng.integers(-2, 3, size=(int(rng.integers(0, 9)), 3)) * int(rng.choice([1, 1, 1 << 20]))
        else:                                                       # every entry at the limit, signs at random
            vectors = rng.choice([-big, big, big - 1, 1 - big], size=(int(rng.integers(3, 6)), 3))
        exp, exp_rank = R.hnf(vectors.tolist())
        ok, rank, rows, fits, basis = hnf_of(probe, vectors)
        assert ok == 1 and rank == exp_rank and rows == exp, (trial, vectors.tolist())
        small = all(-(1 << 31) <= x < (1 << 31) for r in exp for x in r)
        assert fits == int(small) and (not small or basis == exp)
    assert hnf_of(probe, [[big, big, big]])[2][0] == [big, big, big] and hnf_of(probe, [[big, big, big]])[3] == 0     # 2^31 is no int32
    assert hnf_of(probe, [[2, 0, 0]])[4] == [[2, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert hnf_of(probe, [[2, 0, 0], [1, 0, 0]])[4] == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]


def test_quotient_on_records_written_by_hand(probe):
    def quotient(rec, first_full_ends=False):
        out = probe(7, len(rec), int(first_full_ends), np.array(rec, dtype=np.int64).reshape(-1, 3))
        ok, max_rank, cycles, distinct, n_pairs, n_comps = (int(v) for v in out[:6])
        pairs = out[6:6 + 2 * n_pairs].reshape(-1, 2).tolist()
        comps = out[6 + 2 * n_pairs:].reshape(n_comps, 11)
        return ok, max_rank, cycles, distinct, sorted(pairs), [(int(c[0]), int(c[1]), c[2:].reshape(3, 3).tolist()) for c in comps]
    code = lambda s: 9 * (s[0] + 1) + 3 * (s[1] + 1) + s[2] + 1                        # noqa: E731
    assert quotient([]) == (1, 0, 0, 0, [], [])
    # one open component that meets itself across the first axis, recorded four times
    assert quotient([[7, 7, code((1, 0, 0))]] * 4) == (1, 1, 1, 1, [], [(7, 1, [[1, 0, 0], [0, 0, 0], [0, 0, 0]])])
    # two open components, each the other's neighbour across the seam: together once round the cell
    ok, max_rank, cycles, distinct, pairs, comps = quotient([[3, 9, code((1, 0, 0))], [9, 3, code((1, 0, 0))]])
    assert (ok, max_rank, cycles, distinct, pairs) == (1, 1, 1, 2, [[9, 3]]) and comps == [(3, 1, [[2, 0, 0], [0, 0, 0], [0, 0, 0]])]
    # a tree of open components has no loop
    ok, max_rank, cycles, _, pairs, comps = quotient([[5, 2, code((0, 1, 0))], [8, 5, code((0, 0, 1))], [11, 8, code((1, 1, 1))]])
    assert (ok, max_rank, cycles, comps) == (1, 0, 0, []) and pairs == [[5, 2], [8, 2], [11, 2]]
    # lattices of two classes that meet are added; the class keeps the lowest root
    ok, max_rank, _, _, pairs, comps = quotient([[4, 4, code((1, 0, 0))], [6, 6, code((0, 1, 0))], [6, 4, code((0, 0, 1))], [4, 6, code((0, 0, 1))]])
    assert (ok, max_rank, pairs) == (1, 3, [[6, 4]]) and comps == [(4, 3, [[1, 0, 0], [0, 1, 0], [0, 0, 2]])]
    assert quotient([[4, 4, code((1, 0, 0))], [4, 4, code((0, 1, 0))], [4, 4, code((0, 0, 1))], [9, 9, code((0, 1, 1))]], True)[:2] == (1, 3)
    for bad in ([[-1, 2, 14]], [[1, -2, 14]], [[1, 2, 13]], [[1, 2, 27]], [[1, 2, -1]]):
        assert quotient(bad)[0] == 0


def test_snap_rule_of_the_bisection(probe):
    g = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-310, 5e-324, 0.01, S, np.nextafter(S, 1.0), 5.0, 2.0 ** -1074])
    for lo in (5e-324, 1e-310, 0.01, np.nextafter(0.01, 1.0), S, np.nextafter(S, 1.0), 5.0, np.nextafter(5.0, 6.0), np.inf):
        bits = int(np.array([lo]).view(np.int64)[0])
        out = probe(4, len(g), bits, g)
        with np.errstate(invalid="ignore"):
            exp = (g > 0.0) & (g >= lo)
        assert np.array_equal(out[:len(g)].astype(bool), exp)
        with np.errstate(invalid="ignore"):
            under = g[(g > 0.0) & (g < lo)]
        assert out[len(g):].view(np.float64).tolist() == [g[exp].min(), g[exp].max(), under.max() if under.size else 0.0]
        assert R.snap(g, lo) == g[exp].min()
    out = probe(4, 3, 1, np.array([0.0, -3.0, np.nan]))
    assert out.tolist() == [0, 0, 0, 0, 0, 0]                       # no candidate: 0, 0, 0
    out = probe(4, 3, int(np.array([7.0]).view(np.int64)[0]), np.array([1.0, 2.0, np.nan]))
    assert out[:3].tolist() == [0, 0, 0] and out[3:].view(np.float64).tolist() == [0.0, 0.0, 2.0]


def levels(probe, grid, connectivity, tile_first=False):
    g = np.ascontiguousarray(grid, dtype=np.float64)
    out = probe(5, g.size, 100 * int(tile_first) + connectivity, np.array(g.shape, dtype=np.int64), g)
    assert out[0] == 1
    return out[5:8].view(np.float64), out[2:5].astype(np.int32), int(out[1])


def test_levels_by_bisection_are_the_levels_by_enumeration(probe):
    rng = np.random.default_rng(5)
    grids = [saddle_grid(), np.zeros((3, 4, 5)), -np.ones((2, 2, 2)), np.full((1, 1, 1), 1e-310), np.full((2, 3, 1), np.nan),
             rng.integers(0, 40, size=(5, 5, 6)) / 8.0, rng.random((6, 7, 5)) * 1e-300, rng.random((4, 9, 3)) ** 8 * 1e12,
             np.where(rng.random((7, 6, 5)) < 0.3, np.inf, rng.random((7, 6, 5)))]
    grids += [c[1] for c in R.designed()]
    for g in grids:
        for connectivity in (6, 26):
            exp_t, exp_r = R.levels(g, connectivity)
            for tile_first in (False, True):
                t, r, passes = levels(probe, g, connectivity, tile_first)
                assert t.tobytes() == exp_t.tobytes() and np.array_equal(r, exp_r), (g.shape, connectivity)
                assert passes <= 3 * 64 and (passes > 0) == bool(np.any(g > 0.0)) and passes <= 3 * (2 + len(np.unique(g[g > 0.0])))
    t, r, passes = levels(probe, saddle_grid(), 26)
    assert t.tobytes() == np.array([S, 0.01, 0.01]).tobytes() and r.tolist() == [1, 3, 3]


KEYS = ["err", "V", "n_tiles", "lds_bytes", "seam_max", "form", "blocks", "workspace", "layout"]


def plan(probe, n=(17, 16, 33), connectivity=26, form=0, cap=-1):
    got = dict(zip(KEYS, (int(v) for v in probe(6, 0, 0, np.array(list(n) + [connectivity, form, cap], dtype=np.int64)))))
    exp = R.plan(n, connectivity, form)
    if exp is None:
        assert got["err"] == 1
        return None
    assert got["err"] == 0 and got["layout"] == 0
    assert {k: got[k] for k in exp} == exp
    return got


def test_plan_layout_and_every_refusal(probe):
    for n in ((1, 1, 1), (2, 3, 5), (17, 16, 33), (64, 48, 40), (160, 176, 192), (1024, 1024, 128), (1, 1024, 7)):
        for connectivity in (6, 18, 26):
            for cap in (-1, 0, 1, 1 << 16):
                p = plan(probe, n, connectivity, cap=cap)
                assert p["form"] in (1, 2) and p["lds_bytes"] <= 65536 and p["seam_max"] < 1 << 32
    assert plan(probe, form=1)["form"] == 1 and plan(probe, form=2)["form"] == 2
    assert plan(probe, (17, 16, 33))["n_tiles"] == 3 * 2 * 3 and plan(probe, (64, 48, 40))["n_tiles"] == 8 * 6 * 3
    for bad in (dict(n=(0, 4, 4)), dict(n=(4, 1025, 4)), dict(n=(4, 4, -1)), dict(n=(1024, 1024, 129)), dict(connectivity=0),
                dict(connectivity=8), dict(connectivity=27), dict(connectivity=-6), dict(form=3), dict(form=-1)):
        assert plan(probe, **bad) is None, bad
