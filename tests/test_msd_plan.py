"""CPU-only: the decisions of the mean squared displacement (sitator_amd/csrc/msd_plan.h) compiled with the host compiler under
ASan / UBSan into a stand-alone probe, the way test_dpc_plan.py builds its own, and driven over stdin / stdout.  Both compilers are
told -ffp-contract=off, so the arithmetic pinned here is what the kernels evaluate.

The probe walks a series the way the kernels do - chunk by chunk, a thread's four elements, the scan of the group totals, the chunk
offsets - with the header's functions, and tests/msd_ref.py says what must come out, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import msd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: int64 mode, N, K.
#   mode 0: float64 f[N]                                               -> int32 n[N]; float64 residual[N]
#   mode 1: float64 y[N]                                               -> float64 P[N + 1]; int64 chunks     (the squares)
#   mode 2: int32 shift[N]                                             -> int32 sums[N]; int64 chunks
#   mode 3: (K lags) float64 inv_m, P[N + 1], re[K]                    -> float64 s1[K], msd[K]
#   mode 4: int64 n_sel, direct, collective, cap, stage_bits (N = F, K = n_lags) -> int64 out[11]
#           out[10]: msd_layout() for batches of one atom, of atoms_per_batch and of the ragged last batch, on a null base and
#           on a made-up one - 0, or the sum of 1 (the buffer is not head + fixed_bytes + B atom_bytes in both runs), 2 (a
#           piece is not 16-byte aligned), 4 (a piece begins before the bytes the kernels touch of the piece before it end,
#           or ends beyond the buffer)
#   mode 5: float64 cm[9], ci[9], x[N, 3]; int32 n[N, 3]               -> float64 unwrapped[N, 3], frac[N, 3]
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "msd_plan.h"

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }

// a series through the scan as the three kernels run it; out[t] = the inclusive sum at t
template <typename T, class Load> static void scan(int64_t F, Load load, std::vector<T> &out)
{
    const int64_t nc = msd_chunks(F);
    std::vector<T> totals((size_t)nc), offsets((size_t)nc), g(MSD_THREADS), tmp(MSD_THREADS);
    std::vector<T> local((size_t)(nc * MSD_CHUNK)), before((size_t)(nc * MSD_THREADS));
    for (int64_t c = 0; c < nc; c++) {
        for (int j = 0; j < MSD_THREADS; j++) {
            T run = (T)0;
            for (int i = 0; i < MSD_GROUP; i++) {
                const int64_t e = c * MSD_CHUNK + (int64_t)j * MSD_GROUP + i;
                const T v = e < F ? load(e) : (T)0;
                run = i == 0 ? v : run + v;
                local[(size_t)e] = run;
            }
            g[(size_t)j] = run;
        }
        msd_group_scan(g.data(), tmp.data());
        for (int j = 0; j < MSD_THREADS; j++) before[(size_t)(c * MSD_THREADS + j)] = j > 0 ? g[(size_t)(j - 1)] : (T)0;
        totals[(size_t)c] = g[MSD_THREADS - 1];
    }
    T run = (T)0;
    for (int64_t c = 0; c < nc; c++) { offsets[(size_t)c] = run; run = c == 0 ? totals[(size_t)c] : run + totals[(size_t)c]; }
    out.assign((size_t)F, (T)0);
    for (int64_t e = 0; e < F; e++) {
        const int64_t c = e / MSD_CHUNK, j = (e % MSD_CHUNK) / MSD_GROUP;
        out[(size_t)e] = msd_scan_value(offsets[(size_t)c], before[(size_t)(c * MSD_THREADS + j)], local[(size_t)e]);
    }
}

static int layout_of(const MsdPlan &p, const MsdPlanIn &in, int64_t B)
{
    Carve sized = {nullptr, 0}, cv = {(char *)((uintptr_t)1 << 40), 0};
    msd_layout(sized, p, in, B);
    const MsdPieces w = msd_layout(cv, p, in, B);
    const int64_t S = 3 * B, F = in.F, M = in.direct ? 0 : p.sp.M;
    const struct { const void *at; int64_t bytes; } piece[] = {
        {w.status, 8}, {w.atoms, in.n_sel * 8}, {w.lags, in.direct ? in.n_lags * 8 : 0}, {w.coll_y, in.collective ? 3 * F * 8 : 0},
        {w.y, S * F * 8}, {w.images, S * F * 4}, {w.psum, in.direct ? 0 : S * (F + 1) * 8}, {w.totals, S * p.n_chunks * 8},
        {w.buf, S * M * 16}, {w.out, S * in.n_lags * 8}, {w.r4, in.direct ? B * in.n_lags * 8 : 0}};
    int bad = 0;
    if (sized.used != cv.used || cv.used != w.head + p.fixed_bytes + B * p.atom_bytes || w.head % 256) bad |= 1;
    int64_t end = 0;
    for (const auto &q : piece) {
        const int64_t off = (int64_t)((uintptr_t)q.at - (uintptr_t)cv.base);
        if (off % 16) bad |= 2;
        if (off < end) bad |= 4;
        end = off + q.bytes;
    }
    if (end > cv.used || w.head != (int64_t)((uintptr_t)w.coll_y - (uintptr_t)cv.base)) bad |= 4;
    return bad;
}

int main()
{
    int64_t h[3];
    if (fread(h, 8, 3, stdin) != 3) return 2;
    const int64_t mode = h[0], N = h[1], K = h[2];
    if (N < 0 || N > ((int64_t)1 << 40) || K < 0 || K > 10000000) return 3;
    if (mode == 0) {
        std::vector<double> f((size_t)N), res((size_t)N);
        std::vector<int32_t> n((size_t)N);
        if (!rd(f.data(), 8, (size_t)N)) return 2;
        for (int64_t i = 0; i < N; i++) n[(size_t)i] = msd_image(f[(size_t)i], &res[(size_t)i]);
        wr(n.data(), 4, (size_t)N);
        wr(res.data(), 8, (size_t)N);
        return 0;
    }
    if (mode == 1) {
        std::vector<double> y((size_t)N), incl, P((size_t)(N + 1), 0.0);
        if (!rd(y.data(), 8, (size_t)N)) return 2;
        scan<double>(N, [&](int64_t e) { return y[(size_t)e] * y[(size_t)e]; }, incl);
        for (int64_t e = 0; e < N; e++) P[(size_t)(e + 1)] = incl[(size_t)e];
        const int64_t nc = msd_chunks(N);
        wr(P.data(), 8, (size_t)(N + 1));
        wr(&nc, 8, 1);
        return 0;
    }
    if (mode == 2) {
        std::vector<int32_t> s((size_t)N), incl;
        if (!rd(s.data(), 4, (size_t)N)) return 2;
        scan<int32_t>(N, [&](int64_t e) { return s[(size_t)e]; }, incl);
        const int64_t nc = msd_chunks(N);
        wr(incl.data(), 4, (size_t)N);
        wr(&nc, 8, 1);
        return 0;
    }
    if (mode == 3) {
        double inv_m;
        std::vector<double> P((size_t)(N + 1)), re((size_t)K), s1((size_t)K), out((size_t)K);
        if (!rd(&inv_m, 8, 1) || !rd(P.data(), 8, (size_t)(N + 1)) || !rd(re.data(), 8, (size_t)K)) return 2;
        if (K > N) return 3;
        for (int64_t t = 0; t < K; t++) {
            s1[(size_t)t] = msd_s1(P.data(), N, t);
            out[(size_t)t] = msd_combine(s1[(size_t)t], re[(size_t)t], inv_m, N, t);
        }
        wr(s1.data(), 8, (size_t)K);
        wr(out.data(), 8, (size_t)K);
        return 0;
    }
    if (mode == 4) {
        int64_t a[5];
        if (!rd(a, 8, 5)) return 2;
        MsdPlanIn in;
        in.F = N; in.n_lags = K; in.n_sel = a[0]; in.direct = a[1] != 0; in.collective = a[2] != 0; in.workspace_bytes = a[3];
        SpKnobs k;
        k.workspace = SP_DEFAULT_WORKSPACE; k.stage_bits = (int)a[4]; k.lines = SP_MAX_LINES;
        const MsdPlan p = msd_plan(in, k);
        int64_t layout = 0;
        if (!p.err) {
            const int64_t last = in.n_sel > 0 ? in.n_sel - (p.n_batches - 1) * p.atoms_per_batch : 1;
            layout = layout_of(p, in, 1) | layout_of(p, in, p.atoms_per_batch) | layout_of(p, in, last);
        }
        const int64_t out[11] = {p.err ? 1 : 0, p.atoms_per_batch, p.n_batches, p.atom_bytes, p.fixed_bytes, p.workspace, p.n_chunks,
                                 in.direct ? 0 : p.sp.M, in.direct ? 0 : p.sp.npass, MSD_MAX_BATCH, layout};
        wr(out, 8, 11);
        return 0;
    }
    if (mode == 5) {
        double cm[9], ci[9];
        std::vector<double> x((size_t)(3 * N)), xu((size_t)(3 * N)), fr((size_t)(3 * N));
        std::vector<int32_t> n((size_t)(3 * N));
        if (!rd(cm, 8, 9) || !rd(ci, 8, 9) || !rd(x.data(), 8, (size_t)(3 * N)) || !rd(n.data(), 4, (size_t)(3 * N))) return 2;
        for (int64_t i = 0; i < N; i++)
            for (int a = 0; a < 3; a++) {
                const double *p = &x[(size_t)(3 * i)];
                const int32_t *q = &n[(size_t)(3 * i)];
                xu[(size_t)(3 * i + a)] = msd_unwrap(p[a], q[0], q[1], q[2], cm, a);
                fr[(size_t)(3 * i + a)] = msd_frac(ci, a, p[0], p[1], p[2]);
            }
        wr(xu.data(), 8, (size_t)(3 * N));
        wr(fr.data(), 8, (size_t)(3 * N));
        return 0;
    }
    return 3;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("msd_plan")
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


def test_image_rounding(probe):
    half = 0.5
    f = [0.0, -0.0, half, -half, np.nextafter(half, 1.0), np.nextafter(half, 0.0), -np.nextafter(half, 1.0), -np.nextafter(half, 0.0),
         1.5, -1.5, np.nextafter(1.5, 2.0), np.nextafter(1.5, 1.0), 2.5, -2.5, 0.49, 0.51, 3.0, -7.25, 1e-300, 1e9 + 0.5,
         2.0 ** 30, -2.0 ** 30, np.nextafter(2.0 ** 30, 0.0), 1e300, np.nan, np.inf, -np.inf]
    f = np.array(f + list(np.random.default_rng(1).normal(scale=3.0, size=200)))
    raw = probe(0, len(f), 0, f)
    n = np.frombuffer(raw[:4 * len(f)], dtype=np.int32)
    res = np.frombuffer(raw[4 * len(f):], dtype=np.float64)
    exp_n, exp_res = R.image(f)
    assert np.array_equal(n, exp_n)
    assert np.array_equal(bits(res), bits(exp_res))
    assert list(n[:8]) == [0, 0, 0, 0, 1, 0, -1, 0]                                 # ties to even; one ulp either side
    assert list(n[8:14]) == [2, -2, 2, 1, 2, -2]
    assert list(n[20:27]) == [0, 0, 2 ** 30, 0, 0, 0, 0] and np.all(res[[20, 21, 23, 24, 25, 26]] == -1.0)
    finite = res >= 0
    assert res[finite].max() == 0.5 and res[finite].min() == 0.0


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK, 2 * R.CHUNK + 1, 3 * R.CHUNK - 3])
def test_prefix_sums_of_the_squares(probe, F):
    y = np.random.default_rng(F).normal(size=F) * np.linspace(1.0, 30.0, F)
    raw = probe(1, F, 0, y)
    P = np.frombuffer(raw[:8 * (F + 1)], dtype=np.float64)
    chunks = np.frombuffer(raw[8 * (F + 1):], dtype=np.int64)[0]
    assert chunks == R.n_chunks(F) == (1 if F <= R.CHUNK else 2 if F <= 2 * R.CHUNK else 3)
    assert np.array_equal(bits(P), bits(R.prefix_squares(y)))
    exact = np.concatenate([[0.0], np.cumsum(y.astype(np.longdouble) ** 2)])
    assert np.max(np.abs(P - exact)) <= 16 * np.finfo(np.float64).eps * float(exact[-1])


@pytest.mark.parametrize("F", [1, 2, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK + 7])
def test_image_sums(probe, F):
    shift = np.random.default_rng(F).integers(-2, 3, size=F).astype(np.int32)
    raw = probe(2, F, 0, shift)
    sums = np.frombuffer(raw[:4 * F], dtype=np.int32)
    assert np.array_equal(sums, np.cumsum(shift, dtype=np.int32))


def test_windowed_term_and_combination(probe):
    F = 37
    rng = np.random.default_rng(5)
    y = rng.normal(size=F)
    P = R.prefix_squares(y)
    M = R.padded_length(F)
    re = rng.normal(size=F) * M
    raw = probe(3, F, F, np.array([1.0 / M]), P, re)
    s1 = np.frombuffer(raw[:8 * F], dtype=np.float64)
    out = np.frombuffer(raw[8 * F:], dtype=np.float64)
    tau = np.arange(F)
    exp_s1 = R.s1(P, F, tau)
    assert np.array_equal(bits(s1), bits(exp_s1))
    exp = exp_s1 - 2.0 * (re * (1.0 / M)) / (F - tau)
    exp[0] = 0.0
    assert np.array_equal(bits(out), bits(exp))
    # S1 is what it stands for: sum_{t < F - tau} (y[t]^2 + y[t + tau]^2) / (F - tau)
    direct = np.array([np.sum(y[:F - t] ** 2 + y[t:] ** 2) / (F - t) for t in tau])
    np.testing.assert_allclose(s1, direct, rtol=1e-13)


def plan(probe, F, n_lags, n_sel, direct, collective, cap, stage_bits=10):
    out = np.frombuffer(probe(4, F, n_lags, np.array([n_sel, int(direct), int(collective), cap, stage_bits], dtype=np.int64)), dtype=np.int64)
    keys = ["err", "atoms_per_batch", "n_batches", "atom_bytes", "fixed_bytes", "workspace", "n_chunks", "M", "npass", "max_batch",
            "layout"]
    p = dict(zip(keys, (int(v) for v in out)))
    assert len(out) == len(keys) and p["layout"] == 0             # the pieces of msd_layout: the plan's bytes, aligned, apart
    return p


@pytest.mark.parametrize("F,n_lags,direct", [(2, 2, False), (257, 129, False), (513, 513, False), (20000, 10001, False),
                                             (257, 6, True), (100000, 64, True), (524289, 50, False)])
def test_batch_sizing(probe, F, n_lags, direct):
    ab = R.atom_bytes(F, n_lags, direct)
    for collective in (False, True):
        fixed = R.fixed_bytes(F, collective)
        p = plan(probe, F, n_lags, 5, direct, collective, 0)
        assert p["err"] == 0 and p["atom_bytes"] == ab and p["fixed_bytes"] == fixed and p["n_chunks"] == R.n_chunks(F)
        assert p["max_batch"] == R.MAX_BATCH
        if not direct:
            assert p["M"] == R.padded_length(F) and p["npass"] == (1 if p["M"] <= 1024 else 2 if p["M"] <= 1 << 20 else 3)
        for cap in (fixed + ab, fixed + 2 * ab + 100, fixed + 5 * ab, fixed + 1000 * ab):
            p = plan(probe, F, n_lags, 5, direct, collective, cap)
            assert (p["atoms_per_batch"], p["n_batches"]) == R.batch(F, 5, n_lags, direct, collective, cap)
            assert p["workspace"] == fixed + p["atoms_per_batch"] * ab <= cap
        assert plan(probe, F, n_lags, 5, direct, collective, fixed + ab - 1)["err"] == 1
        assert R.batch(F, 5, n_lags, direct, collective, fixed + ab - 1) is None


def test_plan_limits(probe):
    assert plan(probe, 1, 1, 1, False, False, 0)["err"] == 1
    assert plan(probe, (1 << 29) + 1, 1, 1, True, False, 0)["err"] == 1
    assert plan(probe, 100, 0, 1, False, False, 0)["err"] == 1
    assert plan(probe, 100, 5, 0, False, False, 0)["n_batches"] == 0
    p = plan(probe, 2, 2, 10 ** 6, True, False, 1 << 40)
    assert p["atoms_per_batch"] == R.MAX_BATCH and p["n_batches"] == -(-10 ** 6 // R.MAX_BATCH)
    assert plan(probe, 700, 700, 1, False, False, 0, stage_bits=4)["npass"] == 3
    assert plan(probe, 1 << 20, 5, 1, False, False, 0, stage_bits=4)["err"] == 1          # more than three passes


@pytest.mark.parametrize("name", sorted(R.CELLS))
def test_unwrapped_position_and_fractional_step(probe, name):
    cell = R.CELLS[name]
    cm = np.ascontiguousarray(cell.T)
    ci = np.linalg.inv(cm)
    rng = np.random.default_rng(7)
    x = rng.normal(scale=4.0, size=(300, 3))
    x[0] = [-0.0, 0.0, -0.0]
    n = rng.integers(-3, 4, size=(300, 3)).astype(np.int32)
    n[:40] = 0                                                                      # no image: the position itself, also -0.0
    raw = probe(5, len(x), 0, cm, ci, x, n)
    xu = np.frombuffer(raw[:8 * x.size], dtype=np.float64).reshape(-1, 3)
    fr = np.frombuffer(raw[8 * x.size:], dtype=np.float64).reshape(-1, 3)
    nf = n.astype(np.float64)
    exp = np.stack([x[:, a] + ((nf[:, 0] * cm[a, 0] + nf[:, 1] * cm[a, 1]) + nf[:, 2] * cm[a, 2]) for a in range(3)], axis=1)
    exp[:40] = x[:40]
    assert np.array_equal(bits(xu), bits(exp))
    assert np.array_equal(bits(xu[:40]), bits(x[:40]))
    exp_f = np.stack([(ci[a, 0] * x[:, 0] + ci[a, 1] * x[:, 1]) + ci[a, 2] * x[:, 2] for a in range(3)], axis=1)
    assert np.array_equal(bits(fr), bits(exp_f))
    np.testing.assert_allclose(fr, x @ np.linalg.inv(cell), rtol=0, atol=1e-12)     # f = d . cell^-1
    np.testing.assert_allclose(xu, x + n @ cell, rtol=0, atol=1e-12)                # x + N_0 c_0 + N_1 c_1 + N_2 c_2
