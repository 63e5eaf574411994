"""CPU-only: the decisions of EnergyLandscape (sitator_amd/csrc/landscape_plan.h) compiled with the host compiler under ASan / UBSan
into a stand-alone probe, the way test_percolation_plan.py builds its own, and driven over stdin / stdout; tests/landscape_ref.py
says what must come out.  Everything is an integer or the bytes of a double: no tolerance."""
import os
import subprocess

import numpy as np
import pytest

from tests import barrier_ref as BR
from tests import landscape_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: float64 cm[9] (cell.T), ci[9], rc; int64 grid[3], form, mode, S, t; float64 pos[S][3], eps[S], sigma[S]
#   mode 0: -> int64 err, V, n_tiles, form, n[3], wide[3]
#   mode 1: the tiled schedule of tile t (lp_tile_serial) -> int64 chunks, entries; float64 e[256]; int64 live[256] (flat voxel or -1);
#           int64 triples[entries][4]
#   mode 2: the direct form at every voxel -> float64 e[V]; int64 walked[V]
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "landscape_plan.h"

struct Cell { double cm[9], ci[9]; };
static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }
static void wr1(int64_t v) { wr(&v, 8, 1); }

int main()
{
    Cell c; double rc; int64_t h[7];
    if (!rd(c.cm, 8, 9) || !rd(c.ci, 8, 9) || !rd(&rc, 8, 1) || !rd(h, 8, 7)) return 2;
    const int64_t mode = h[4], S = h[5], t = h[6];
    if (S < 0 || S > 100000) return 3;
    const LandscapePlan p = lp_plan(c, rc, h, (int)h[3]);
    if (mode == 0) {
        wr1(p.err ? 1 : 0); wr1(p.V); wr1(p.n_tiles); wr1(p.form);
        for (int a = 0; a < 3; a++) wr1(p.err ? 0 : p.bp.n[a]);
        for (int a = 0; a < 3; a++) wr1(p.wide[a]);
        return 0;
    }
    if (p.err) return 4;
    std::vector<double> pos(3 * S), eps(S), sigma(S), atoms(S * BP_REC);
    if (!rd(pos.data(), 8, 3 * S) || !rd(eps.data(), 8, S) || !rd(sigma.data(), 8, S)) return 2;
    for (int64_t s = 0; s < S; s++) bp_atom(c, pos.data() + 3 * s, eps[s], sigma[s], rc, atoms.data() + s * BP_REC);
    if (mode == 1) {
        if (t < 0 || t >= p.n_tiles) return 3;
        double e[LP_BLOCK];
        int64_t chunks, entries;
        lp_tile_serial<LpLJ>(c, p, atoms.data(), S, t, e, &chunks, &entries, nullptr);
        std::vector<int64_t> triples(4 * entries);
        lp_tile_serial<LpLJ>(c, p, atoms.data(), S, t, e, &chunks, &entries, triples.data());
        wr1(chunks); wr1(entries);
        wr(e, 8, LP_BLOCK);
        const LpTile tl = lp_tile(p, t);
        for (int x = 0; x < LP_BLOCK; x++) {
            int64_t i[3];
            wr1(lp_tile_voxel(tl, x, i) ? (i[0] * p.n[1] + i[1]) * p.n[2] + i[2] : -1);
        }
        wr(triples.data(), 8, triples.size());
        return 0;
    }
    if (mode == 2) {
        std::vector<double> e(p.V);
        std::vector<int64_t> walked(p.V);
        for (int64_t v = 0; v < p.V; v++) {
            const int64_t i[3] = {v / (p.n[1] * p.n[2]), v / p.n[2] % p.n[1], v % p.n[2]};
            const double f[3] = {lp_frac(i[0], p.n[0]), lp_frac(i[1], p.n[1]), lp_frac(i[2], p.n[2])};
            double x[3];
            lp_center(c, f, x);
            e[v] = 0.0; walked[v] = 0;
            for (int64_t s = 0; s < S; s++) walked[v] += lp_atom_add<LpLJ>(c, p.bp, atoms.data() + s * BP_REC, x, f, e[v]);
        }
        wr(e.data(), 8, e.size()); wr(walked.data(), 8, walked.size());
        return 0;
    }
    return 3;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("landscape_plan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])

    def run(cell, rc, grid, form=0, mode=0, pos=None, eps=None, sigma=None, t=0):
        cell = np.asarray(cell, dtype=np.float64)
        S = 0 if pos is None else len(pos)
        with np.errstate(all="ignore"):
            ci = np.linalg.inv(cell.T) if abs(np.linalg.det(cell)) > 0 else np.zeros((3, 3))
        data = np.ascontiguousarray(cell.T).tobytes() + np.ascontiguousarray(ci).tobytes() + np.array([rc], dtype=np.float64).tobytes() \
            + np.array(list(grid) + [form, mode, S, t], dtype=np.int64).tobytes()
        if S:
            data += b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in (pos, eps, sigma))
        return subprocess.run([exe], input=data, stdout=subprocess.PIPE, check=True).stdout
    return run


def lattice(cell, S, seed):
    rng = np.random.default_rng(seed)
    pos = rng.random((S, 3)) @ cell
    pos[0] += np.array([1.0, -2.0, 0.0]) @ cell                    # one atom outside the cell
    return pos, 0.5 + rng.random(S), 0.8 + 0.4 * rng.random(S)


CASES = [(name, grid, S, rcf) for name in ("CUBIC", "TRICLINIC", "SMALL_TRICLINIC")
         for grid, S, rcf in (((2, 3, 5), 4, 0.3), ((1, 1, 2), 3, 2.2), ((5, 9, 10), 5, 1.0))] + [("SMALL_TRICLINIC", (5, 9, 10), 5, 2.2)]


@pytest.mark.parametrize("name, grid, S, rcf", CASES, ids=["%s-%s-%d-%g" % (c[0], "x".join(str(v) for v in c[1]), c[2], c[3]) for c in CASES])
def test_every_tile_lists_all_terms_in_order_and_sums_to_the_restatement(probe, name, grid, S, rcf):
    cell = getattr(BR, name)
    rc = rcf * BR.heights(cell).min()
    pos, eps, sigma = lattice(cell, S, 3 + S)
    want = LR.energies(cell, pos, eps, sigma, rc, grid)
    V = grid[0] * grid[1] * grid[2]
    nt = LR.n_tiles(grid)
    n_tiles = nt[0] * nt[1] * nt[2]
    seen, partial, most_chunks = np.zeros(V, dtype=bool), 0, 0
    for t in range(n_tiles):
        out = probe(cell, rc, grid, mode=1, pos=pos, eps=eps, sigma=sigma, t=t)
        chunks, entries = np.frombuffer(out[:16], dtype=np.int64)
        e = np.frombuffer(out[16:16 + 8 * 256], dtype=np.float64)
        live = np.frombuffer(out[16 + 8 * 256:16 + 16 * 256], dtype=np.int64)
        triples = np.frombuffer(out[16 + 16 * 256:], dtype=np.int64).reshape(-1, 4)
        vox, is_partial = LR.tile_voxels(grid, t)
        partial += is_partial
        assert sorted(live[live >= 0].tolist()) == sorted(vox.tolist()) and (len(vox) < 256) == is_partial
        assert len(triples) == entries and chunks == -(-entries // LR.CHUNK)
        most_chunks = max(most_chunks, int(chunks))
        keys = [tuple(int(v) for v in r) for r in triples]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)                    # ascending (s, m0, m1, m2)
        listed = set(keys)
        for v in vox:
            _, _, atom, m = LR.voxel_terms(cell, pos, eps, sigma, rc, LR.center(cell, grid, LR.unflatten(grid, int(v))))
            assert {(int(a),) + tuple(int(k) for k in mm) for a, mm in zip(atom, m)} <= listed
        own = live >= 0
        assert e[own].tobytes() == want[live[own]].tobytes() and not e[~own].any()
        seen[live[own]] = True
    assert seen.all() and (partial > 0) == any(grid[a] % LR.TILE[a] for a in range(3))
    if rcf > 2 and grid == (5, 9, 10):
        assert most_chunks >= 2                                   # the list of a tile runs over several chunks
    direct = probe(cell, rc, grid, mode=2, pos=pos, eps=eps, sigma=sigma)
    assert direct[:8 * V] == want.tobytes()
    assert np.frombuffer(direct[8 * V:], dtype=np.int64).min() >= 0


def test_an_atom_on_a_voxel_centre_is_plus_infinity_in_both_schedules(probe):
    cell, grid = BR.TRICLINIC, (3, 5, 7)
    on = LR.center(cell, grid, (1, 4, 2))
    pos = np.array([on, on + 0.37 * cell[0]])
    rc = 0.45 * BR.heights(cell).min()
    v = (1 * 5 + 4) * 7 + 2
    direct = np.frombuffer(probe(cell, rc, grid, mode=2, pos=pos, eps=[1.0, 0.7], sigma=[1.0, 1.2])[:8 * 105], dtype=np.float64)
    assert direct[v] == np.inf and np.isinf(direct).sum() == 1 and not np.isnan(direct).any()
    out = probe(cell, rc, grid, mode=1, pos=pos, eps=[1.0, 0.7], sigma=[1.0, 1.2], t=0)
    e = np.frombuffer(out[16:16 + 8 * 256], dtype=np.float64)
    live = np.frombuffer(out[16 + 8 * 256:16 + 16 * 256], dtype=np.int64)
    assert e[live == v] == np.inf and e[live >= 0].tobytes() == direct[live[live >= 0]].tobytes()


def plan(probe, cell=BR.TRICLINIC, rc=3.0, grid=(17, 16, 33), form=0):
    got = np.frombuffer(probe(cell, rc, grid, form=form), dtype=np.int64)
    exp = LR.plan(cell, rc, grid, form)
    if exp is None:
        assert got[0] == 1
        return None
    assert got[0] == 0 and got[1] == exp["voxels"] and got[2] == exp["tiles"] and got[3] == exp["form"]
    assert tuple(got[4:7]) == exp["translations"] and tuple(got[7:10]) == exp["list_translations"]
    return got


def test_plan_and_every_refusal(probe):
    for cell in (BR.CUBIC, BR.TRICLINIC, BR.SMALL_TRICLINIC):
        for grid in ((1, 1, 1), (2, 3, 5), (17, 16, 33), (8, 16, 16), (1024, 1024, 128), (1, 1024, 7)):
            for rcf in (0.3, 0.4, 1.05, 2.2, 100.3):
                for form in (0, 1, 2):
                    assert plan(probe, cell, rcf * BR.heights(cell).min(), grid, form) is not None
    assert plan(probe, grid=(17, 16, 33))[2] == 5 * 2 * 5 and plan(probe, grid=(8, 16, 16))[2] == 8
    flat = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
    for bad in (dict(grid=(0, 4, 4)), dict(grid=(4, 1025, 4)), dict(grid=(4, 4, -1)), dict(grid=(1024, 1024, 129)), dict(form=3), dict(form=-1),
                dict(cell=flat), dict(rc=0.0), dict(rc=-1.0), dict(rc=np.inf), dict(rc=np.nan),
                dict(cell=BR.SMALL_TRICLINIC, rc=256.0 * BR.heights(BR.SMALL_TRICLINIC).min())):
        assert plan(probe, **bad) is None, bad
    assert plan(probe, cell=BR.SMALL_TRICLINIC, rc=254.0 * BR.heights(BR.SMALL_TRICLINIC).min(), grid=(2, 2, 2)) is not None
