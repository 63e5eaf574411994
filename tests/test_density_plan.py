"""CPU-only: the decisions of the ionic density (sitator_amd/csrc/density_plan.h) compiled with the host compiler under ASan /
UBSan into a stand-alone probe, the way test_scattering_plan.py builds its own, and driven over stdin / stdout.  Both compilers
are told -ffp-contract=off, so the arithmetic pinned here is what the kernels evaluate; tests/density_ref.py says what must come
out, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import density_ref as R
from tests import msd_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: int64 mode, N, K.
#   mode 0: float64 ci[9]; int64 n[3]; float64 p[N, 3]     -> int64 dn_voxel[N]
#   mode 1: (K = n) float64 s[N]                           -> int64 dn_axis[N]
#   mode 2: (K = n_classes) int32 site_class[N]; int64 labels[N] (each in [-1, N)) -> int64 dn_plane[N]
#   mode 3: (K = probes) int64 key[N]                      -> int64 slot[N][K]: dn_probe(dn_slot(key), i)
#   mode 4: int64 n[3]; float64 threshold; float64 grid[N] -> int64 dn_is_peak[N]
#   mode 5: int64 F, A, n_sel, stride, n0, n1, n2, K, n_classes, n_taps, h0, h1, h2, form, host, cap -> int64 out[16]
#           out[15]: dn_layout() on a null base and on a made-up one - 0, or the sum of 1 (the two runs disagree, or the work area
#           is not the plan's `workspace` bytes behind `head`, or it is beyond the cap), 2 (a piece is not 256-byte aligned), 4 (a
#           piece begins before the bytes the kernels touch of the piece before it end, or ends beyond the buffer)
#   mode 6: int64 n[3]; int64 taps[N, 3]                   -> int64 ok, halo[3]
#   mode 7: (K = lo .. hi as two further int64) int64 list[N] -> int64 dn_first_outside
#   mode 8: float64 (cm[9], ci[9])[N]                      -> int64 dn_cell_ok[N]
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "density_plan.h"

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }

static int layout_of(const DnPlan &p, const DnPlanIn &in, int64_t cap)
{
    Carve sized = {nullptr, 0}, cv = {(char *)((uintptr_t)1 << 40), 0};
    dn_layout(sized, p, in);
    const DnPieces w = dn_layout(cv, p, in);
    struct Piece { const void *at; int64_t bytes; };
    const Piece pieces[] = {{w.atoms, in.n_sel * 8}, {w.site_class, in.K * 4}, {w.taps, in.n_taps * 12}, {w.weights, in.n_taps * 8},
                            {w.status, 32}, {w.counts, p.cells * 8}, {w.smoothed, in.n_taps > 0 ? p.cells * 8 : 0},
                            {w.upload, in.host ? p.window_frames * in.A * 24 : 0}};
    int bad = 0;
    if (sized.used != cv.used || cv.used != w.head + p.workspace || w.head % 256 || (in.host && p.workspace > cap)) bad |= 1;
    if (!in.host && p.workspace != 0) bad |= 1;
    int64_t end = 0;
    for (int i = 0; i < 8; i++) {
        const int64_t off = (int64_t)((uintptr_t)pieces[i].at - (uintptr_t)cv.base);
        if (off % 256) bad |= 2;
        if (off < end || (i == 7 && off != w.head)) bad |= 4;
        end = off + pieces[i].bytes;
        if (i == 6 && end > w.head) bad |= 4;
    }
    if (end > cv.used) bad |= 4;
    return bad;
}

int main()
{
    int64_t h[3];
    if (fread(h, 8, 3, stdin) != 3) return 2;
    const int64_t mode = h[0], N = h[1], K = h[2];
    if (N < 0 || N > 10000000 || K < 0 || K > 10000000) return 3;
    const size_t n = (size_t)N;
    if (mode == 0) {
        double ci[9]; int64_t g[3];
        std::vector<double> p(3 * n);
        std::vector<int64_t> v(n);
        if (!rd(ci, 8, 9) || !rd(g, 8, 3) || !rd(p.data(), 8, 3 * n)) return 2;
        for (size_t i = 0; i < n; i++) v[i] = dn_voxel(ci, g, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
        wr(v.data(), 8, n);
        return 0;
    }
    if (mode == 1) {
        std::vector<double> s(n);
        std::vector<int64_t> v(n);
        if (!rd(s.data(), 8, n)) return 2;
        for (size_t i = 0; i < n; i++) v[i] = dn_axis(s[i], K);
        wr(v.data(), 8, n);
        return 0;
    }
    if (mode == 2) {
        std::vector<int32_t> sc(n);
        std::vector<int64_t> l(n), v(n);
        if (!rd(sc.data(), 4, n) || !rd(l.data(), 8, n)) return 2;
        for (size_t i = 0; i < n; i++) {
            if (l[i] < -1 || l[i] >= N) return 3;
            v[i] = dn_plane(l[i], sc.data(), K);
        }
        wr(v.data(), 8, n);
        return 0;
    }
    if (mode == 3) {
        std::vector<int64_t> key(n), v(n * (size_t)K);
        if (!rd(key.data(), 8, n)) return 2;
        for (size_t i = 0; i < n; i++)
            for (int64_t j = 0; j < K; j++) v[i * (size_t)K + (size_t)j] = dn_probe(dn_slot((uint32_t)key[i]), (int)j);
        wr(v.data(), 8, v.size());
        return 0;
    }
    if (mode == 4) {
        int64_t g[3]; double threshold;
        if (!rd(g, 8, 3) || !rd(&threshold, 8, 1)) return 2;
        if (g[0] < 1 || g[1] < 1 || g[2] < 1 || g[0] * g[1] * g[2] != N) return 3;
        std::vector<double> grid(n);
        std::vector<int64_t> v(n);
        if (!rd(grid.data(), 8, n)) return 2;
        for (size_t i = 0; i < n; i++) v[i] = dn_is_peak(grid.data(), g, (int64_t)i, threshold) ? 1 : 0;
        wr(v.data(), 8, n);
        return 0;
    }
    if (mode == 5) {
        int64_t a[16];
        if (!rd(a, 8, 16)) return 2;
        DnPlanIn in;
        in.F = a[0]; in.A = a[1]; in.n_sel = a[2]; in.stride = a[3]; in.n[0] = a[4]; in.n[1] = a[5]; in.n[2] = a[6]; in.K = a[7];
        in.n_classes = a[8]; in.n_taps = a[9]; in.halo[0] = a[10]; in.halo[1] = a[11]; in.halo[2] = a[12]; in.form = a[13];
        in.host = a[14] != 0; in.workspace_bytes = a[15];
        const DnPlan p = dn_plan(in, SP_DEFAULT_WORKSPACE);
        const int64_t out[16] = {p.err ? 1 : 0, p.V, p.cells, p.taken, p.runs, p.form, p.lds_bytes, p.window, p.n_windows, p.window_frames,
                                 p.ext[0], p.ext[1], p.ext[2], p.smooth_lds, p.workspace,
                                 p.err ? 0 : layout_of(p, in, a[15] > 0 ? a[15] : SP_DEFAULT_WORKSPACE)};
        wr(out, 8, 16);
        return 0;
    }
    if (mode == 6) {
        int64_t g[3], out[4];
        std::vector<int64_t> taps(3 * n);
        if (!rd(g, 8, 3) || !rd(taps.data(), 8, 3 * n)) return 2;
        out[0] = dn_halo(taps.data(), N, g, out + 1) ? 1 : 0;
        wr(out, 8, 4);
        return 0;
    }
    if (mode == 7) {
        int64_t range[2];
        std::vector<int64_t> list(n);
        if (!rd(range, 8, 2) || !rd(list.data(), 8, n)) return 2;
        const int64_t at = dn_first_outside(list.data(), N, range[0], range[1]);
        wr(&at, 8, 1);
        return 0;
    }
    if (mode == 8) {
        std::vector<double> m(18 * n);
        std::vector<int64_t> v(n);
        if (!rd(m.data(), 8, 18 * n)) return 2;
        for (size_t i = 0; i < n; i++) v[i] = dn_cell_ok(&m[18 * i], &m[18 * i + 9]) ? 1 : 0;
        wr(v.data(), 8, n);
        return 0;
    }
    return 3;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("density_plan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])

    def run(mode, N, K, *arrays):
        data = np.array([mode, N, K], dtype=np.int64).tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
        return np.frombuffer(subprocess.run([exe], input=data, stdout=subprocess.PIPE, check=True).stdout, dtype=np.int64)
    return run


DESIGNED_S = np.array([-1e-17, 1.0 - 2.0 ** -53, -2.0 ** -60, 5.0 - 2.0 ** -50, -0.0, 0.0, 1.0, -1.0, 0.5, 1e300, -1e300, 4503599627370497.0,
                       np.nan, np.inf, -np.inf])


@pytest.mark.parametrize("n", [1, 3, 7, 8, 1024])
def test_axis_index_at_the_designed_arguments(probe, n):
    k = np.arange(n)
    s = np.concatenate([DESIGNED_S, k / np.float64(n), np.nextafter(k / np.float64(n), -np.inf), k / np.float64(n) - 7.0,
                        np.random.default_rng(n).uniform(-50, 50, 5000)])
    got = probe(1, len(s), n, s)
    assert np.array_equal(got, R.axis_index(s, n))
    assert list(got[:4]) == [n - 1] * 4 and list(got[4:8]) == [0] * 4 and list(got[12:15]) == [-1] * 3
    fin = np.isfinite(s)
    assert got[fin].min() >= 0 and got[fin].max() <= n - 1


@pytest.mark.parametrize("name", sorted(M.CELLS))
def test_voxel_bit_for_bit_over_three_cells(probe, name):
    cell = M.CELLS[name]
    ci = R.cell_inverse(cell)
    rng = np.random.default_rng(17)
    for grid in ((1, 1, 1), (2, 3, 5), (17, 16, 33), (1024, 7, 64)):
        k = np.stack(np.meshgrid(*[np.arange(min(g, 9)) for g in grid], indexing="ij"), axis=-1).reshape(-1, 3)
        on_faces = (k / np.asarray(grid, dtype=np.float64)) @ cell              # at (or an ulp from) voxel boundaries
        pts = np.concatenate([on_faces, on_faces + 3.0 * cell[0] - 2.0 * cell[2], rng.uniform(-30, 30, (100000, 3)),
                              [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e308, 1e308, 1e308], [-1e-17, -1e-17, -1e-17]]])
        got = probe(0, len(pts), 0, ci, np.array(grid, dtype=np.int64), pts)
        exp = R.voxel(pts, ci, grid)
        assert np.array_equal(got, exp)
        V = grid[0] * grid[1] * grid[2]
        assert got.max() <= V - 1 and got.min() == -1 and list(got[-5:-2]) == [-1] * 3 and got[-1] >= 0


def test_class_map(probe):
    sc = np.array([0, 2, 1, 0, 14, 3], dtype=np.int32)
    labels = np.array([-1, 0, 1, 2, 3, 4], dtype=np.int64)
    got = probe(2, 6, 16, sc, labels)
    assert list(got) == [15, 0, 2, 1, 0, 14] and np.array_equal(got, R.plane(labels, sc, 16))


def test_hash_slot_and_probe_sequence(probe):
    keys = np.concatenate([[0, 1, 2, (1 << 27) - 1, 12345], np.random.default_rng(2).integers(0, 1 << 27, 2000)]).astype(np.int64)
    got = probe(3, len(keys), R.PROBE, keys).reshape(len(keys), R.PROBE)
    exp = np.array([[R.probe(R.slot(k), i) for i in range(R.PROBE)] for k in keys])
    assert np.array_equal(got, exp) and got.min() >= 0 and got.max() < R.SLOTS
    assert all(len(set(row)) == R.PROBE for row in got)               # a probe sequence visits distinct slots
    first = got[5:, 0]
    assert np.bincount(first, minlength=R.SLOTS).max() <= 8              # and the first slots spread
    run = probe(3, 64, 1, np.arange(1000, 1064, dtype=np.int64))[:]      # consecutive voxels do not share a first slot
    assert len(set(run)) == 64


def test_peak_rule_on_small_grids(probe):
    rng = np.random.default_rng(9)
    grids = []
    for shape in ((1, 1, 1), (1, 1, 2), (2, 2, 2), (1, 4, 2), (3, 3, 3), (5, 4, 6), (2, 1, 7)):
        grids.append(rng.integers(0, 4, size=shape).astype(float))   # many ties
        grids.append(rng.normal(size=shape))
        grids.append(np.zeros(shape))
        withnan = rng.integers(0, 3, size=shape).astype(float)
        withnan.reshape(-1)[rng.integers(0, withnan.size)] = np.nan
        grids.append(withnan)
    blobs = np.zeros((9, 8, 7))
    blobs[2, 2, 2], blobs[2, 2, 3], blobs[6, 5, 1], blobs[6, 6, 1] = 5.0, 3.0, 4.0, 1.0
    grids.append(blobs)
    for g in grids:
        for thr in (0.0, 0.5, -np.inf, np.nan):
            got = probe(4, g.size, 0, np.array(g.shape, dtype=np.int64), np.array([thr]), g)
            assert np.array_equal(np.flatnonzero(got), R.peaks(g, thr)), (g.shape, thr)
    assert list(np.flatnonzero(probe(4, blobs.size, 0, np.array(blobs.shape, dtype=np.int64), np.array([0.5]), blobs))) == [128, 372]


KEYS = ["err", "V", "cells", "taken", "runs", "form", "lds_bytes", "window", "n_windows", "window_frames", "ext0", "ext1", "ext2",
        "smooth_lds", "workspace", "layout"]


def plan(probe, F=389, A=140, n_sel=130, stride=1, grid=(17, 16, 33), K=0, n_classes=1, n_taps=0, halo=(0, 0, 0), form=0, host=True, cap=0):
    got = dict(zip(KEYS, (int(v) for v in probe(5, 0, 0, np.array([F, A, n_sel, stride, grid[0], grid[1], grid[2], K, n_classes, n_taps,
                                                                  halo[0], halo[1], halo[2], form, host, cap], dtype=np.int64)))))
    exp = R.plan(F, A, n_sel, grid, stride, K, n_classes, n_taps, halo, form, host, cap)
    if exp is None:
        assert got["err"] == 1
        return None
    assert got["err"] == 0 and got["layout"] == 0
    ext = exp.pop("ext")
    assert [got["ext0"], got["ext1"], got["ext2"]] == ext
    assert {k: got[k] for k in exp} == exp
    assert got["form"] in (1, 2) and (form == 0 or got["form"] == form) and got["lds_bytes"] <= 65536 and got["smooth_lds"] <= R.SMOOTH_LDS
    assert got["window"] >= 1 and (got["window"] == got["taken"] or got["window"] % R.RUN == 0)
    return got


@pytest.mark.parametrize("F,A,n_sel,stride", [(1, 1, 1, 1), (389, 140, 130, 1), (389, 140, 130, 3), (100000, 576, 64, 1), (1000, 3, 2, 5000),
                                              (6500, 70, 64, 100)])
def test_windows_and_layout_for_caps_from_one_run_to_everything(probe, F, A, n_sel, stride):
    base = plan(probe, F, A, n_sel, stride, host=False)
    assert base["workspace"] == 0 and base["window"] == base["taken"] == (F - 1) // stride + 1 and base["n_windows"] == 1
    first = min(base["taken"], R.RUN)
    one = -(-(((first - 1) * stride + 1) * A * 24) // 256) * 256
    assert plan(probe, F, A, n_sel, stride, cap=one - 1) is None
    least = plan(probe, F, A, n_sel, stride, cap=one)
    assert least["window"] == first and least["n_windows"] == base["runs"]
    seen = set()
    for cap in (one + 5, 2 * one + 300, 3 * one + 7, 17 * one, 1 << 24, 1 << 30, 1 << 40):
        p = plan(probe, F, A, n_sel, stride, cap=cap, n_taps=5, halo=(1, 2, 0), K=7, n_classes=3)
        assert p["workspace"] <= cap and p["window_frames"] <= F
        seen.add(p["window"])
    whole = plan(probe, F, A, n_sel, stride, cap=1 << 50)
    assert whole["window"] == whole["taken"] and whole["n_windows"] == 1
    assert len(seen) >= 2 or base["runs"] <= 2


def test_smoothing_tile_and_halo(probe):
    assert plan(probe, n_taps=0)["smooth_lds"] == 0
    p = plan(probe, n_taps=1)
    assert (p["ext0"], p["ext1"], p["ext2"], p["smooth_lds"]) == (4, 8, 8, 2048)
    p = plan(probe, grid=(64, 48, 40), n_taps=925, halo=(6, 6, 6))
    assert (p["ext0"], p["ext1"], p["ext2"], p["smooth_lds"]) == (16, 20, 20, 51200)
    assert plan(probe, grid=(64, 48, 40), n_taps=925, halo=(7, 7, 7))["smooth_lds"] == 0          # 18 x 22 x 22 doubles: beyond the LDS tile
    assert plan(probe, grid=(64, 48, 40), n_taps=9, halo=(31, 0, 0))["smooth_lds"] == 66 * 8 * 8 * 8 and R.SMOOTH_LDS < 65536


def test_every_refusal_of_the_validation(probe):
    assert plan(probe) is not None
    for bad in (dict(grid=(0, 4, 4)), dict(grid=(4, 1025, 4)), dict(grid=(4, 4, -1)), dict(n_classes=0), dict(n_classes=17, K=3),
                dict(grid=(1024, 1024, 129)), dict(grid=(1024, 1024, 9), n_classes=16, K=1), dict(F=0), dict(F=(1 << 29) + 1), dict(stride=0),
                dict(stride=-4), dict(n_sel=0), dict(n_sel=(1 << 20) + 1), dict(A=0), dict(n_taps=-1), dict(n_taps=(1 << 15) + 1),
                dict(n_taps=3, halo=(9, 0, 0)), dict(n_taps=3, halo=(0, 8, 0)), dict(n_taps=3, halo=(0, 0, 17)), dict(n_taps=3, halo=(-1, 0, 0)),
                dict(form=3), dict(form=-1), dict(cap=-1), dict(cap=255), dict(K=-1), dict(K=5, n_classes=1),
                dict(cap=64 * 140 * 24 - 1)):
        assert plan(probe, **bad) is None, bad
    assert plan(probe, n_taps=3, halo=(8, 7, 16)) is not None and plan(probe, form=1)["form"] == 1 and plan(probe, form=2)["form"] == 2
    assert plan(probe, grid=(16, 16, 16))["form"] == 2 and plan(probe, grid=(16, 16, 17))["form"] == 1          # form 0: a slot per key, or direct
    assert plan(probe, grid=(16, 16, 8), K=4, n_classes=2)["form"] == 2 and plan(probe, grid=(16, 16, 8), K=4, n_classes=3)["form"] == 1
    assert plan(probe, F=1 << 29, A=1 << 20, n_sel=1 << 20, grid=(1024, 1024, 128), n_taps=1 << 15, host=False) is not None
    assert plan(probe, grid=(1024, 1024, 8), n_classes=16, K=1 << 30, host=False) is not None
    assert plan(probe, grid=(16, 16, 33), n_taps=3, halo=(8, 0, 0)) is None                        # (16 - 1) / 2 = 7

    def halo(taps, grid):
        t = np.array(taps, dtype=np.int64).reshape(-1, 3)
        got = probe(6, len(t), 0, np.array(grid, dtype=np.int64), t)
        exp = R.halo(t, grid)
        assert (got[0] == 0) == (exp is None) and (exp is None or list(got[1:]) == exp)
        return None if got[0] == 0 else list(got[1:])
    assert halo([[1, -2, 0], [0, 1, 3]], (5, 5, 7)) == [1, 2, 3] and halo([], (1, 1, 1)) == [0, 0, 0] and halo([[0, 0, 0]], (1, 1, 1)) == [0, 0, 0]
    assert halo([[0, 0, 4]], (5, 5, 7)) is None and halo([[-3, 0, 0]], (6, 5, 7)) is None and halo([[1, 0, 0]], (2, 5, 7)) is None
    assert halo([[0, 0, 1 << 40]], (5, 5, 7)) is None and halo([[-2, 2, -3]], (5, 5, 7)) == [2, 2, 3]

    def outside(values, lo, hi):
        arr = np.array(values, dtype=np.int64)
        return probe(7, len(arr), 0, np.array([lo, hi], dtype=np.int64), arr)[0]
    assert outside([0, 5, 9], 0, 9) == -1 and outside([], 0, 9) == -1
    assert outside([0, 10, -1], 0, 9) == 1 and outside([-1], 0, 9) == 0 and outside([3, 1 << 40], 0, 9) == 1

    cells = [M.ORTHO, M.HEX, M.TRICLINIC, np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [5.0, 7.0, 9.0]]), np.zeros((3, 3))]
    rows = []
    for c in cells:
        with np.errstate(all="ignore"):
            try:
                ci = np.linalg.inv(c.T)
            except np.linalg.LinAlgError:
                ci = np.full((3, 3), np.inf)
        rows.append(np.concatenate([c.T.reshape(-1), ci.reshape(-1)]))
    bad_inverse = np.concatenate([M.ORTHO.T.reshape(-1), np.full(9, np.nan)])
    got = probe(8, len(rows) + 1, 0, np.array(rows + [bad_inverse]))
    assert list(got) == [1, 1, 1, 0, 0, 0]
