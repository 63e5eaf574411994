"""CPU-only: the decisions of the van Hove correlation function (sitator_amd/csrc/vanhove_plan.h) compiled with the host
compiler under ASan / UBSan into a stand-alone probe, the way test_msd_plan.py builds its own, and driven over stdin / stdout.
Both compilers are told -ffp-contract=off, so the arithmetic pinned here is what the kernels evaluate; tests/vanhove_ref.py
says what must come out, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import msd_ref as R
from tests import vanhove_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: int64 mode, N, K.
#   mode 0: (K = n_bins) float64 r_max, r2[N]; int64 guess[N]        -> float64 e2[K + 1]; int64 bin[N], int64 kernel_guess_bin[N]
#   mode 1: int64 (F, tau, stride)[N]                                -> int64 origins[N]
#   mode 2: int64 F, n_a, n_b, n_lags, n_bins, stride, self, distinct, unwrap, cap, copies -> int64 out[12]
#           out[11]: vh_layout() on a null base and on a made-up one - 0, or the sum of 1 (the two runs disagree, or the work
#           area is not the plan's `workspace` bytes behind `head`), 2 (a piece is not 256-byte aligned), 4 (a piece begins before
#           the bytes the kernels touch of the piece before it end, or ends beyond the buffer; the two uses of the work area
#           are walked one after the other)
#   mode 3: float64 ci[9], r_max[N]                                  -> float64 hmin; int64 ok[N]
#   mode 4: float64 cm[9], ci[9], xa[N, 3], xb[N, 3]                 -> float64 r2[N]
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "vanhove_plan.h"

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }

static int layout_of(const VhPlan &p, const VhPlanIn &in)
{
    Carve sized = {nullptr, 0}, cv = {(char *)((uintptr_t)1 << 40), 0};
    vh_layout(sized, p, in);
    const VhPieces w = vh_layout(cv, p, in);
    const int64_t table = in.n_lags * (in.n_bins + 1) * 8, S = 3 * p.self_batch, F = in.F;
    const bool s = in.want_self, d = in.want_distinct, u = in.want_self && in.unwrap;
    struct Piece { const void *at; int64_t bytes; };
    const Piece head[] = {{w.status, 8}, {w.atoms, (in.n_a + in.n_b) * 8}, {w.lags, in.n_lags * 8}, {w.e2, (in.n_bins + 1) * 8},
                          {w.self_counts, s ? table : 0}, {w.distinct_counts, d ? table : 0}};
    const Piece use_d[] = {{w.sa, d ? p.window * 3 * in.n_a * 8 : 0}, {w.sb, d ? p.window * 3 * in.n_b * 8 : 0}};
    const Piece use_s[] = {{w.y, s ? S * F * 8 : 0}, {w.images, u ? S * F * 4 : 0}, {w.totals, u ? S * p.n_chunks * 8 : 0}};
    int bad = 0;
    if (sized.used != cv.used || cv.used != w.head + p.workspace || w.head % 256) bad |= 1;
    int64_t end = 0;
    const auto walk = [&](const Piece *q, int n, int64_t from) {
        end = from;
        for (int i = 0; i < n; i++) {
            const int64_t off = (int64_t)((uintptr_t)q[i].at - (uintptr_t)cv.base);
            if (off % 256) bad |= 2;
            if (off < end) bad |= 4;
            end = off + q[i].bytes;
        }
        if (end > cv.used) bad |= 4;
    };
    walk(head, 6, 0);
    if (end > w.head) bad |= 4;
    walk(use_d, 2, w.head);
    walk(use_s, 3, w.head);
    return bad;
}

int main()
{
    int64_t h[3];
    if (fread(h, 8, 3, stdin) != 3) return 2;
    const int64_t mode = h[0], N = h[1], K = h[2];
    if (N < 0 || N > 10000000 || K < 0 || K > 10000000) return 3;
    if (mode == 0) {
        double r_max;
        std::vector<double> r2((size_t)N), e2((size_t)(K + 1));
        std::vector<int64_t> guess((size_t)N), bin((size_t)N), kbin((size_t)N);
        if (!rd(&r_max, 8, 1) || !rd(r2.data(), 8, (size_t)N) || !rd(guess.data(), 8, (size_t)N)) return 2;
        vh_edges2(r_max, K, e2.data());
        const float inv_dr = (float)((double)K / r_max);
        for (int64_t i = 0; i < N; i++) {
            bin[(size_t)i] = vh_bin(r2[(size_t)i], e2.data(), K, guess[(size_t)i]);
            kbin[(size_t)i] = r2[(size_t)i] >= 0.0 && r2[(size_t)i] < e2[(size_t)K] ? vh_bin(r2[(size_t)i], e2.data(), K, vh_guess(r2[(size_t)i], inv_dr)) : K;
        }
        wr(e2.data(), 8, (size_t)(K + 1));
        wr(bin.data(), 8, (size_t)N);
        wr(kbin.data(), 8, (size_t)N);
        return 0;
    }
    if (mode == 1) {
        std::vector<int64_t> in((size_t)(3 * N)), out((size_t)N);
        if (!rd(in.data(), 8, (size_t)(3 * N))) return 2;
        for (int64_t i = 0; i < N; i++) out[(size_t)i] = vh_origins(in[(size_t)(3 * i)], in[(size_t)(3 * i + 1)], in[(size_t)(3 * i + 2)]);
        wr(out.data(), 8, (size_t)N);
        return 0;
    }
    if (mode == 2) {
        int64_t a[11];
        if (!rd(a, 8, 11)) return 2;
        VhPlanIn in;
        in.F = a[0]; in.n_a = a[1]; in.n_b = a[2]; in.n_lags = a[3]; in.n_bins = a[4]; in.stride = a[5];
        in.want_self = a[6] != 0; in.want_distinct = a[7] != 0; in.unwrap = a[8] != 0; in.workspace_bytes = a[9]; in.hist_copies = (int)a[10];
        const VhPlan p = vh_plan(in, SP_DEFAULT_WORKSPACE);
        const int64_t out[12] = {p.err ? 1 : 0, p.run, p.b_span, p.b_tiles, p.pairs_per_wg, p.window, p.origins_per_window, p.self_batch,
                                 p.n_chunks, p.lds_bytes, p.workspace, p.err ? 0 : layout_of(p, in)};
        wr(out, 8, 12);
        return 0;
    }
    if (mode == 3) {
        double ci[9];
        std::vector<double> r((size_t)N);
        std::vector<int64_t> ok((size_t)N);
        if (!rd(ci, 8, 9) || !rd(r.data(), 8, (size_t)N)) return 2;
        const double hm = vh_hmin(ci);
        for (int64_t i = 0; i < N; i++) ok[(size_t)i] = vh_rmax_ok(r[(size_t)i], hm) ? 1 : 0;
        wr(&hm, 8, 1);
        wr(ok.data(), 8, (size_t)N);
        return 0;
    }
    if (mode == 4) {
        double cm[9], ci[9];
        std::vector<double> xa((size_t)(3 * N)), xb((size_t)(3 * N)), r2((size_t)N);
        if (!rd(cm, 8, 9) || !rd(ci, 8, 9) || !rd(xa.data(), 8, (size_t)(3 * N)) || !rd(xb.data(), 8, (size_t)(3 * N))) return 2;
        for (int64_t i = 0; i < N; i++) {
            const double *p = &xa[(size_t)(3 * i)], *q = &xb[(size_t)(3 * i)];
            double ds[3];
            for (int a = 0; a < 3; a++) ds[a] = msd_frac(ci, a, q[0], q[1], q[2]) - msd_frac(ci, a, p[0], p[1], p[2]);
            r2[(size_t)i] = vh_image_r2(ds[0], ds[1], ds[2], cm);
        }
        wr(r2.data(), 8, (size_t)N);
        return 0;
    }
    return 3;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("vanhove_plan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])

    def run(mode, N, K, *arrays):
        data = np.array([mode, N, K], dtype=np.int64).tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
        return subprocess.run([exe], input=data, stdout=subprocess.PIPE, check=True).stdout
    return run


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("r_max,n_bins", [(2.0, 1), (1.7, 16), (2.6749999, 300), (0.3, 2048), (1e-3, 7), (3e5, 33)])
def test_bin_walk_at_every_edge_from_a_wrong_guess(probe, r_max, n_bins):
    """e2[k] and the doubles either side of it for every k, zero, values beyond, NaN and the infinities - each from a guess that is
    deliberately wrong (0, the last bin, far outside on both sides, random) and from the kernels' own guess."""
    exp_e2 = V.edges2(r_max, n_bins)
    pts = np.concatenate([exp_e2, np.nextafter(exp_e2, -np.inf), np.nextafter(exp_e2, np.inf), [0.0, -0.0, 5e-324, r_max * r_max * 4, 1e300,
                          np.nan, np.inf, -np.inf, -1.0], np.random.default_rng(3).random(200) * r_max * r_max * 1.2])
    rng = np.random.default_rng(4)
    for guess in (np.zeros(len(pts)), np.full(len(pts), n_bins - 1), np.full(len(pts), -(1 << 40)), np.full(len(pts), 1 << 40),
                  rng.integers(-5, n_bins + 5, size=len(pts))):
        raw = probe(0, len(pts), n_bins, np.array([r_max]), pts, guess.astype(np.int64))
        e2 = np.frombuffer(raw[:8 * (n_bins + 1)], dtype=np.float64)
        rest = np.frombuffer(raw[8 * (n_bins + 1):], dtype=np.int64)
        got, kernel = rest[:len(pts)], rest[len(pts):]
        assert np.array_equal(bits(e2), bits(exp_e2)) and np.all(np.diff(e2) >= 0)
        exp = V.bin_of(pts, exp_e2)
        assert np.array_equal(got, exp) and np.array_equal(kernel, exp)
    tail = exp[3 * (n_bins + 1):3 * (n_bins + 1) + 9]
    assert list(tail) == [0, 0, 0] + [n_bins] * 6                 # NaN, the infinities and a negative value: overflow
    assert exp[n_bins] == n_bins and exp[2 * n_bins + 1] == n_bins - 1      # r_max^2 itself is out, the double below it is in


def test_origins(probe):
    cases = [(F, tau, s) for F in (1, 2, 3, 10, 97, 400) for tau in sorted({0, 1, F // 2, F - 1}) if tau < F for s in (1, 2, 3, 7, 1000)]
    got = np.frombuffer(probe(1, len(cases), 0, np.array(cases, dtype=np.int64)), dtype=np.int64)
    for (F, tau, s), n in zip(cases, got):
        assert n == V.n_origins(F, tau, s) == len(range(0, F - tau, s)) >= 1


KEYS = ["err", "run", "b_span", "b_tiles", "pairs_per_wg", "window", "origins_per_window", "self_batch", "n_chunks", "lds_bytes",
        "workspace", "layout"]


def plan(probe, F, n_a, n_b, n_lags=3, n_bins=16, stride=1, self_part=True, distinct_part=True, unwrap=True, cap=0, copies=1):
    raw = probe(2, 0, 0, np.array([F, n_a, n_b, n_lags, n_bins, stride, self_part, distinct_part, unwrap, cap, copies], dtype=np.int64))
    p = dict(zip(KEYS, (int(v) for v in np.frombuffer(raw, dtype=np.int64))))
    assert p["layout"] == 0                                       # the pieces of vh_layout: the plan's bytes, aligned, apart
    return p


@pytest.mark.parametrize("n_a,n_b", [(1, 1), (5, 70), (33, 200), (64, 64), (64, 512), (1000, 1000), (16384, 17), (1 << 20, 1 << 20),
                                     (1, 1 << 20), (300, 100000)])
def test_pairs_per_workgroup_stay_below_the_counter(probe, n_a, n_b):
    p = plan(probe, 100, n_a, n_b, self_part=False)
    run, span, tiles, pairs = V.split(n_a, n_b)
    assert (p["run"], p["b_span"], p["b_tiles"], p["pairs_per_wg"]) == (run, span, tiles, pairs)
    assert p["err"] == 0 and 1 <= pairs < 2 ** 32 and pairs <= V.MAX_PAIRS and span % 64 == 0 and run >= 1
    assert tiles * span >= n_b and (tiles - 1) * span < n_b and tiles <= 65535


@pytest.mark.parametrize("F,n_a,n_b,n_bins,stride,unwrap", [(1, 1, 1, 1, 1, True), (96, 7, 70, 16, 1, True), (400, 33, 200, 300, 3, False),
                                                           (100000, 64, 64, 300, 10, True), (100000, 64, 512, 2048, 1, True)])
def test_windows_batches_and_layout(probe, F, n_a, n_b, n_bins, stride, unwrap):
    frame = (n_a + n_b) * 24
    for copies in (1, 4):
        for sp, dp in ((True, True), (True, False), (False, True)):
            for cap in (0, 512 + frame, 512 + 3 * frame + 5, 768 + 3 * (R.round256(F * 8) + R.round256(F * 4) + 256) * 2, 1 << 40):
                raw_cap = cap if cap else 1 << 30
                w = V.window(F, n_a, n_b, raw_cap) if dp else F
                b = V.self_batch(F, n_a, unwrap, raw_cap) if sp else 0
                raw = probe(2, 0, 0, np.array([F, n_a, n_b, 3, n_bins, stride, sp, dp, unwrap, cap, copies], dtype=np.int64))
                p = dict(zip(KEYS, (int(v) for v in np.frombuffer(raw, dtype=np.int64))))
                if w is None or b is None:
                    assert p["err"] == 1
                    continue
                assert p["err"] == 0 and p["layout"] == 0
                assert (p["window"], p["self_batch"], p["origins_per_window"]) == (w, b, (w - 1) // stride + 1)
                assert p["lds_bytes"] == V.lds_bytes(n_bins, copies) < 65536 and p["n_chunks"] == R.n_chunks(F)
                assert p["workspace"] <= raw_cap
    assert plan(probe, F, n_a, n_b, n_bins=n_bins, cap=511 + frame, self_part=False)["err"] == 1      # below one window


def test_plan_limits(probe):
    ok = dict(F=10, n_a=3, n_b=4)
    assert plan(probe, **ok)["err"] == 0
    for bad in (dict(F=0), dict(F=(1 << 29) + 1), dict(n_lags=0), dict(stride=0), dict(n_bins=0), dict(n_bins=2049), dict(n_a=0),
                dict(n_b=0), dict(n_a=(1 << 20) + 1), dict(self_part=False, distinct_part=False), dict(copies=2), dict(cap=600)):
        assert plan(probe, **dict(ok, **bad))["err"] == 1, bad
    assert plan(probe, **dict(ok, n_bins=2048, copies=4))["lds_bytes"] == V.lds_bytes(2048, 4) < 65536


@pytest.mark.parametrize("name", sorted(R.CELLS))
def test_r_max_check_and_height(probe, name):
    cell = R.CELLS[name]
    _, ci = V.cell_matrices(cell)
    h = V.hmin(cell)
    limit = 0.5 * h * V.MARGIN
    r = np.array([limit, np.nextafter(limit, 0.0), np.nextafter(limit, 10.0), 0.5 * h, 1e-300, 0.0, -1.0, np.nan, np.inf, 1.0])
    raw = probe(3, len(r), 0, ci, r)
    assert np.frombuffer(raw[:8], dtype=np.float64)[0] == h
    np.testing.assert_allclose(h, R.heights(cell).min(), rtol=1e-14)
    ok = np.frombuffer(raw[8:], dtype=np.int64)
    assert list(ok) == [int(V.rmax_ok(v, h)) for v in r] == [1, 1, 0, 0, 1, 0, 0, 0, 0, 1]
    raw = probe(3, 1, 0, np.zeros(9), np.array([1.0]))             # a cell without an inverse: no r_max is right
    assert np.frombuffer(raw[8:], dtype=np.int64)[0] == 0


@pytest.mark.parametrize("name", sorted(R.CELLS))
def test_image_of_a_pair(probe, name):
    cell = R.CELLS[name]
    cm, ci = V.cell_matrices(cell)
    rng = np.random.default_rng(8)
    xa, xb = rng.uniform(-4.0, 4.0, size=(500, 3)), rng.uniform(-4.0, 4.0, size=(500, 3))   # at most three cells apart
    xb[0] = xa[0]                                                 # the same point: 0
    xb[1] = xa[1] + 0.5 * cell[0]                                 # half a cell vector away
    xb[2, 1] = np.nan
    xb[3, 0] = np.inf
    got = np.frombuffer(probe(4, len(xa), 0, cm, ci, xa, xb), dtype=np.float64)
    exp = V.image_r2(V.fractional(xb, ci) - V.fractional(xa, ci), cm)
    assert np.array_equal(bits(got), bits(exp))
    assert got[0] == 0.0 and np.isnan(got[2]) and np.isnan(got[3])
    np.testing.assert_allclose(got[1], np.sum(cell[0] ** 2) / 4.0, rtol=1e-9)
    n = np.arange(-4, 5)
    shifts = np.stack(np.meshgrid(n, n, n, indexing="ij"), axis=-1).reshape(-1, 3) @ cell
    brute = np.min(np.sum(((xb - xa)[4:, None, :] + shifts[None]) ** 2, axis=2), axis=1)
    near = got[4:] < (0.5 * V.hmin(cell)) ** 2
    np.testing.assert_allclose(got[4:][near], brute[near], rtol=1e-11)
