"""CPU-only: the decisions of the intermediate scattering function (sitator_amd/csrc/scattering_plan.h) compiled with the host
compiler under ASan / UBSan into a stand-alone probe, the way test_vanhove_plan.py builds its own, and driven over stdin / stdout.
Both compilers are told -ffp-contract=off, so the arithmetic pinned here is what the kernels evaluate; tests/scattering_ref.py
says what must come out, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import scattering_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: int64 mode, N, K.
#   mode 0: float64 s[N]                                   -> float64 sc_reduce[N]
#   mode 1: float64 f[N]                                   -> float64 cos[N], sin[N]
#   mode 2: (K = H) float64 (c, s)[N]                      -> float64 tab[N][2 (K + 1)]
#   mode 3: (K = n_q) float64 f[N, 3]; int64 q[K, 3]       -> int64 ok, H[3]; float64 (re, im)[N, K] (nothing beyond H where not ok)
#   mode 4: int64 (F, tau, stride)[N]                      -> int64 origins[N], blocks[N]
#   mode 5: float64 v[N, SC_BLOCK]                         -> float64 sc_tree[N]
#   mode 6: int64 F, n_a, n_b, same, n_q, H0, H1, H2, n_lags, stride, self, coherent, cap -> int64 out[12]
#           out[11]: sc_layout() on a null base and on a made-up one - 0, or the sum of 1 (the two runs disagree, or the work
#           area is not the plan's `workspace` bytes behind `head`, or it is beyond the cap), 2 (a piece is not 256-byte aligned),
#           4 (a piece begins before the bytes the kernels touch of the piece before it end, or ends beyond the buffer)
#   mode 7: (K = lo .. hi as two further int64) int64 list[N] -> int64 sc_first_outside
#   mode 8: float64 (a, b)[N]; float64 (ar, ai, br, bi)[N] -> float64 sc_delta[N]; float64 sc_cross (re, im)[N]
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "scattering_plan.h"

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }

static int layout_of(const ScPlan &p, const ScPlanIn &in, int64_t cap)
{
    Carve sized = {nullptr, 0}, cv = {(char *)((uintptr_t)1 << 40), 0};
    sc_layout(sized, p, in);
    const ScPieces w = sc_layout(cv, p, in);
    const int64_t table = in.n_lags * in.n_q * 16;
    const bool s = in.want_self, c = in.want_coherent;
    struct Piece { const void *at; int64_t bytes; };
    const Piece pieces[] = {{w.atoms, (in.n_a + in.n_b) * 8}, {w.lags, in.n_lags * 8}, {w.q, in.n_q * 12}, {w.self_sums, s ? table : 0},
                            {w.coherent_sums, c ? table : 0},
                            {w.frac, c ? p.window * 3 * p.n_cols * 8 : 0}, {w.rho, c ? p.n_sel * p.q_batch * in.F * 16 : 0},
                            {w.partial, p.lags_per_launch * p.n_blocks * p.q_batch * 16}};
    int bad = 0;
    if (sized.used != cv.used || cv.used != w.head + p.workspace || w.head % 256 || p.workspace > cap) bad |= 1;
    int64_t end = 0;
    for (int i = 0; i < 8; i++) {
        const int64_t off = (int64_t)((uintptr_t)pieces[i].at - (uintptr_t)cv.base);
        if (off % 256) bad |= 2;
        if (off < end || (i == 5 && off != w.head)) bad |= 4;
        end = off + pieces[i].bytes;
        if (i == 4 && end > w.head) bad |= 4;
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
    const size_t n = (size_t)N, k = (size_t)K;
    if (mode == 0) {
        std::vector<double> s(n), f(n);
        if (!rd(s.data(), 8, n)) return 2;
        for (size_t i = 0; i < n; i++) f[i] = sc_reduce(s[i]);
        wr(f.data(), 8, n);
        return 0;
    }
    if (mode == 1) {
        std::vector<double> f(n), c(n), s(n);
        if (!rd(f.data(), 8, n)) return 2;
        for (size_t i = 0; i < n; i++) sc_sincos2pi(f[i], &c[i], &s[i]);
        wr(c.data(), 8, n);
        wr(s.data(), 8, n);
        return 0;
    }
    if (mode == 2) {
        if (K > SC_MAX_H) return 3;
        std::vector<double> e(2 * n), tab(n * 2 * (k + 1));
        if (!rd(e.data(), 8, 2 * n)) return 2;
        for (size_t i = 0; i < n; i++) sc_powers(e[2 * i], e[2 * i + 1], (int)K, &tab[i * 2 * (k + 1)]);
        wr(tab.data(), 8, tab.size());
        return 0;
    }
    if (mode == 3) {
        std::vector<double> f(3 * n), out(2 * n * k);
        std::vector<int64_t> q(3 * k);
        if (!rd(f.data(), 8, 3 * n) || !rd(q.data(), 8, 3 * k)) return 2;
        int64_t head[4];
        head[0] = sc_hmax(q.data(), K, head + 1) ? 1 : 0;
        wr(head, 8, 4);
        if (!head[0]) return 0;
        std::vector<double> t0(2 * (size_t)(head[1] + 1)), t1(2 * (size_t)(head[2] + 1)), t2(2 * (size_t)(head[3] + 1));
        for (size_t i = 0; i < n; i++) {
            double c, s;
            sc_sincos2pi(f[3 * i], &c, &s); sc_powers(c, s, (int)head[1], t0.data());
            sc_sincos2pi(f[3 * i + 1], &c, &s); sc_powers(c, s, (int)head[2], t1.data());
            sc_sincos2pi(f[3 * i + 2], &c, &s); sc_powers(c, s, (int)head[3], t2.data());
            for (size_t j = 0; j < k; j++)
                sc_term(t0.data(), t1.data(), t2.data(), (int)q[3 * j], (int)q[3 * j + 1], (int)q[3 * j + 2], &out[2 * (i * k + j)],
                        &out[2 * (i * k + j) + 1]);
        }
        wr(out.data(), 8, out.size());
        return 0;
    }
    if (mode == 4) {
        std::vector<int64_t> in(3 * n), out(2 * n);
        if (!rd(in.data(), 8, 3 * n)) return 2;
        for (size_t i = 0; i < n; i++) {
            out[i] = sc_origins(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
            out[n + i] = sc_blocks(out[i]);
        }
        wr(out.data(), 8, 2 * n);
        return 0;
    }
    if (mode == 5) {
        std::vector<double> v(n * SC_BLOCK), out(n);
        if (!rd(v.data(), 8, v.size())) return 2;
        for (size_t i = 0; i < n; i++) out[i] = sc_tree(&v[i * SC_BLOCK]);
        wr(out.data(), 8, n);
        return 0;
    }
    if (mode == 6) {
        int64_t a[13];
        if (!rd(a, 8, 13)) return 2;
        ScPlanIn in;
        in.F = a[0]; in.n_a = a[1]; in.n_b = a[2]; in.same = a[3] != 0; in.n_q = a[4]; in.H[0] = a[5]; in.H[1] = a[6]; in.H[2] = a[7];
        in.n_lags = a[8]; in.stride = a[9]; in.want_self = a[10] != 0; in.want_coherent = a[11] != 0; in.workspace_bytes = a[12];
        const ScPlan p = sc_plan(in, SP_DEFAULT_WORKSPACE);
        const int64_t out[12] = {p.err ? 1 : 0, p.n_sel, p.n_cols, p.row, p.tile, p.lds_bytes, p.n_blocks, p.q_batch, p.window,
                                 p.lags_per_launch, p.workspace, p.err ? 0 : layout_of(p, in, a[12] > 0 ? a[12] : SP_DEFAULT_WORKSPACE)};
        wr(out, 8, 12);
        return 0;
    }
    if (mode == 7) {
        int64_t range[2];
        std::vector<int64_t> list(n);
        if (!rd(range, 8, 2) || !rd(list.data(), 8, n)) return 2;
        const int64_t at = sc_first_outside(list.data(), N, range[0], range[1]);
        wr(&at, 8, 1);
        return 0;
    }
    if (mode == 8) {
        std::vector<double> ab(2 * n), z(4 * n), d(n), x(2 * n);
        if (!rd(ab.data(), 8, 2 * n) || !rd(z.data(), 8, 4 * n)) return 2;
        for (size_t i = 0; i < n; i++) {
            d[i] = sc_delta(ab[2 * i], ab[2 * i + 1]);
            sc_cross(z[4 * i], z[4 * i + 1], z[4 * i + 2], z[4 * i + 3], &x[2 * i], &x[2 * i + 1]);
        }
        wr(d.data(), 8, n);
        wr(x.data(), 8, 2 * n);
        return 0;
    }
    return 3;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("scattering_plan")
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


def same_bits(got, exp):
    """Bit for bit; a NaN need only be a NaN."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    nan = np.isnan(exp)
    return got.shape == exp.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(exp[~nan]))


def around(values):
    v = np.asarray(values, dtype=np.float64)
    return np.concatenate([v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)])


def test_reduction_at_the_ties_and_beyond(probe):
    s = np.concatenate([around([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.0, 1.0, -1.0, 1e15 + 0.5, 4503599627370496.0]),
                        [np.nan, np.inf, -np.inf, 1e300, -0.0], np.random.default_rng(1).uniform(-40.0, 40.0, 1000)])
    got = np.frombuffer(probe(0, len(s), 0, s), dtype=np.float64)
    assert same_bits(got, S.reduce(s))
    assert got[0] == 0.5 and got[1] == -0.5 and got[2] == -0.5 and got[3] == 0.5          # ties to even: 0, 0, 2, -2
    fin = np.isfinite(s)
    assert np.all(np.abs(got[fin]) <= 0.5) and np.all(np.isnan(got[~fin]))
    assert np.all(got[fin] + np.rint(s[fin]) == s[fin])                                  # exact


DESIGNED = around([0.0, 0.125, -0.125, 0.25, -0.25, 0.375, -0.375, 0.5, -0.5, 1.0, -1.0])


def test_sincos_bit_for_bit_and_at_the_designed_arguments(probe):
    f = np.concatenate([DESIGNED, [np.nan, np.inf, -np.inf, 1.5, -3.0, -0.0], np.random.default_rng(2).uniform(-0.5, 0.5, 100000)])
    raw = np.frombuffer(probe(1, len(f), 0, f), dtype=np.float64)
    c, s = raw[:len(f)], raw[len(f):]
    ec, es = S.sincos2pi(f)
    assert same_bits(c, ec) and same_bits(s, es)
    n = len(DESIGNED) // 3
    assert list(c[:n]) == [1.0, c[1], c[1], 0.0, 0.0, -c[1], -c[1], -1.0, -1.0, 1.0, 1.0]  # exact on the axes, symmetric on the diagonals
    assert list(s[:n]) == [0.0, s[1], -s[1], 1.0, -1.0, s[1], -s[1], 0.0, 0.0, 0.0, 0.0]
    assert abs(c[1] - np.sqrt(0.5)) <= (S.E_SINCOS + 0.5) * S.U and abs(s[1] - np.sqrt(0.5)) <= (S.E_SINCOS + 0.5) * S.U
    beyond = np.abs(f) > 1.0
    assert np.all(np.isnan(c[beyond | np.isnan(f)])) and np.all(np.isnan(s[beyond | np.isnan(f)])) and beyond.sum() >= 5
    ok = np.abs(f) <= 1.0
    xc, xs = S.exact_unit(f[ok])
    err = np.sqrt(((c[ok] - xc) ** 2 + (s[ok] - xs) ** 2).astype(np.float64)) / S.U
    assert err.max() <= S.E_SINCOS


def test_power_table_to_32(probe):
    f = np.concatenate([DESIGNED[np.abs(DESIGNED) <= 0.5], np.random.default_rng(3).uniform(-0.5, 0.5, 300)])
    c, s = S.sincos2pi(f)
    for H in (0, 1, 5, 32):
        raw = np.frombuffer(probe(2, len(f), H, np.stack([c, s], axis=1)), dtype=np.float64).reshape(len(f), H + 1, 2)
        re, im = S.powers(c, s, H)
        assert same_bits(raw[:, :, 0], re) and same_bits(raw[:, :, 1], im)
        assert np.all(raw[:, 0, 0] == 1.0) and np.all(raw[:, 0, 1] == 0.0)
    m = np.arange(33)
    xr, xi = S.exact_unit(f[:, None] * m[None, :])
    err = np.sqrt(((re - xr) ** 2 + (im - xi) ** 2).astype(np.float64))
    assert np.all(err <= S.U * (S.C1 * m)[None, :] * (1 + 2.0 ** -20) + 0.0)


def test_terms_of_a_q_list(probe):
    rng = np.random.default_rng(4)
    q = np.concatenate([[[0, 0, 0], [32, 0, 0], [0, -32, 0], [0, 0, 32], [-32, 32, -32], [1, -2, 3]], rng.integers(-32, 33, size=(60, 3))])
    f = np.concatenate([rng.uniform(-0.5, 0.5, (200, 3)), [[0.5, -0.5, 0.25], [0.0, 0.0, 0.0], [np.nan, 0.1, 0.2]]])
    raw = probe(3, len(f), len(q), f, q.astype(np.int64))
    head = np.frombuffer(raw[:32], dtype=np.int64)
    assert list(head) == [1] + S.h_max(q)
    out = np.frombuffer(raw[32:], dtype=np.float64).reshape(len(f), len(q), 2)
    re, im = S.term(S.tables(f, q), q)
    assert same_bits(out[:, :, 0], re) and same_bits(out[:, :, 1], im)
    assert np.all(out[:-1, 0, 0] == 1.0) and np.all(out[:-1, 0, 1] == 0.0) and np.all(np.isnan(out[-1, 1]))
    assert np.all(np.isnan(out[-1, 0]))                               # (0, 0, 0) too: P_0 of the axis that is not finite is NaN
    xr, xi = S.exact_term(f[:-1], q)
    err = np.sqrt(((re[:-1] - xr) ** 2 + (im[:-1] - xi) ** 2).astype(np.float64))
    assert np.all(err <= S.term_bound(q)[None, :])
    for bad in ([[33, 0, 0]], [[0, 0, -33]], [[1, 2, 3], [0, 1 << 40, 0]]):
        assert np.frombuffer(probe(3, 0, len(bad), np.array(bad, dtype=np.int64))[:8], dtype=np.int64)[0] == 0


def test_origins_and_blocks_at_every_edge(probe):
    cases = [(F, tau, s) for F in (1, 2, 5, 127, 128, 129, 130, 255, 256, 257, 1000) for tau in sorted({0, 1, F // 2, F - 1}) if tau < F
             for s in (1, 2, 3, 1000)]
    got = np.frombuffer(probe(4, len(cases), 0, np.array(cases, dtype=np.int64)), dtype=np.int64)
    for i, (F, tau, s) in enumerate(cases):
        n = got[i]
        assert n == S.n_origins(F, tau, s) == len(range(0, F - tau, s)) >= 1
        assert got[len(cases) + i] == S.n_blocks(n) == -(-n // S.BLOCK)
    assert S.n_blocks(128) == 1 and S.n_blocks(129) == 2


def test_the_tree_of_a_block(probe):
    rng = np.random.default_rng(5)
    v = rng.normal(size=(50, S.BLOCK)) * 10.0 ** rng.integers(-8, 8, size=(50, S.BLOCK))
    v[0] = 0.0
    v[1, 5:] = 0.0                                                    # a ragged last block: the origins beyond count as +0
    v[2, 7] = np.nan
    got = np.frombuffer(probe(5, len(v), 0, v), dtype=np.float64)
    assert same_bits(got, S.tree(v))
    assert not np.array_equal(bits(got[3:]), bits(np.cumsum(v[3:], axis=1)[:, -1]))      # and it is not the running sum
    x = np.zeros((1, S.BLOCK))
    x[0, [0, 64, 32, 96]] = [1.0, 2.0 ** -53, 2.0 ** -53, 1.0]       # the first step adds lanes 64 apart: 1 + 2^-53 twice, lost both times
    assert np.frombuffer(probe(5, 1, 0, x), dtype=np.float64)[0] == 2.0


KEYS = ["err", "n_sel", "n_cols", "row", "tile", "lds_bytes", "n_blocks", "q_batch", "window", "lags_per_launch", "workspace", "layout"]


def plan(probe, F=100, n_a=3, n_b=4, same=False, n_q=10, H=(2, 3, 4), n_lags=3, stride=1, self_part=True, coherent_part=True, cap=0):
    raw = probe(6, 0, 0, np.array([F, n_a, n_b, same, n_q, H[0], H[1], H[2], n_lags, stride, self_part, coherent_part, cap], dtype=np.int64))
    got = dict(zip(KEYS, (int(v) for v in np.frombuffer(raw, dtype=np.int64))))
    exp = S.plan(F, n_a, n_b, same, n_q, list(H), n_lags, stride, self_part, coherent_part, cap)
    if exp is None:
        assert got["err"] == 1
        return None
    assert got["err"] == 0 and got["layout"] == 0
    assert exp.pop("n_q_batches") == -(-n_q // got["q_batch"])
    assert {k: got[k] for k in exp} == exp
    assert got["lds_bytes"] < 65536 and 1 <= got["tile"] <= S.TILE_MAX and got["q_batch"] >= 1 and got["lags_per_launch"] >= 1
    return got


@pytest.mark.parametrize("F,n_a,n_b,same,n_q,H,n_lags", [(1, 1, 1, True, 1, (0, 0, 0), 1), (97, 5, 70, False, 300, (3, 4, 5), 4),
                                                        (129, 130, 130, True, 40, (32, 32, 32), 3), (100000, 64, 64, True, 257, (6, 6, 6), 59),
                                                        (100000, 64, 512, False, 1 << 16, (32, 1, 0), 1)])
def test_batches_windows_and_layout_for_caps_from_one_q_to_everything(probe, F, n_a, n_b, same, n_q, H, n_lags):
    for sp, cp in ((True, True), (True, False), (False, True)):
        base = plan(probe, F, n_a, n_b, same, n_q, H, n_lags, 1, sp, cp)
        n_sel, cols, blocks = base["n_sel"], base["n_cols"], base["n_blocks"]
        one = 1024 + (n_sel * F * 16 + cols * 24 if cp else 0) + blocks * 16
        assert plan(probe, F, n_a, n_b, same, n_q, H, n_lags, 1, sp, cp, cap=one - 1) is None
        least = plan(probe, F, n_a, n_b, same, n_q, H, n_lags, 1, sp, cp, cap=one)
        assert least["q_batch"] == 1 and least["lags_per_launch"] == 1 and least["window"] == (1 if cp else 0)
        seen = set()
        for cap in (one + 5, 3 * one, 17 * one + 3, 1 << 24, 1 << 30, 1 << 40):
            if cap < one:
                continue
            p = plan(probe, F, n_a, n_b, same, n_q, H, n_lags, 1, sp, cp, cap=cap)
            assert p["workspace"] <= cap and (not cp or 1 <= p["window"] <= F)
            seen.add((p["q_batch"], p["window"], p["lags_per_launch"]))
        whole = plan(probe, F, n_a, n_b, same, n_q, H, n_lags, 1, sp, cp, cap=1 << 50)
        assert (whole["q_batch"], whole["lags_per_launch"]) == (min(n_q, S.MAX_QBATCH), n_lags) and whole["window"] == (F if cp else 0)
        assert len(seen) >= 2 or F == 1


def test_tile_and_lds(probe):
    assert plan(probe, H=(0, 0, 0))["tile"] == 64 and plan(probe, H=(32, 32, 32))["tile"] == S.TILE_LDS // (99 * 16) == 15
    assert plan(probe, H=(7, 7, 7))["tile"] == 64 and plan(probe, H=(8, 8, 8))["tile"] == 56
    assert plan(probe, H=(0, 0, 0))["lds_bytes"] == S.LAG_TILE * S.BLOCK * 16                 # the tree of k_sc_coherent is the larger
    assert plan(probe, H=(32, 32, 32))["lds_bytes"] == 15 * 99 * 16


def test_every_refusal_of_the_validation(probe):
    assert plan(probe) is not None
    for bad in (dict(F=0), dict(F=(1 << 29) + 1), dict(n_lags=0), dict(stride=0), dict(stride=-2), dict(n_q=0), dict(n_q=(1 << 16) + 1),
                dict(H=(33, 0, 0)), dict(H=(0, 0, 33)), dict(H=(0, -1, 0)), dict(n_a=0), dict(n_b=0), dict(n_a=(1 << 20) + 1),
                dict(n_b=(1 << 20) + 1), dict(same=True), dict(self_part=False, coherent_part=False), dict(cap=-1), dict(cap=1000),
                dict(cap=1024 + 2 * 100 * 16 + 7 * 24 + 16 - 1)):
        assert plan(probe, **bad) is None, bad
    assert plan(probe, cap=1024 + 2 * 100 * 16 + 7 * 24 + 16)["q_batch"] == 1
    assert plan(probe, F=1 << 29, n_q=1 << 16, H=(32, 32, 32), n_a=1 << 20, n_b=1 << 20, same=True, coherent_part=False) is not None

    def outside(values, lo, hi):
        arr = np.array(values, dtype=np.int64)
        return np.frombuffer(probe(7, len(arr), 0, np.array([lo, hi], dtype=np.int64), arr), dtype=np.int64)[0]
    assert outside([0, 5, 9], 0, 9) == -1 and outside([], 0, 9) == -1
    assert outside([0, 10, -1], 0, 9) == 1 and outside([-1], 0, 9) == 0 and outside([3, 1 << 40], 0, 9) == 1


def test_displacement_and_cross_product(probe):
    rng = np.random.default_rng(6)
    ab = np.concatenate([rng.uniform(-0.5, 0.5, (500, 2)), [[0.5, -0.5], [-0.5, 0.5], [0.25, -0.25], [0.5, 0.0], [np.nan, 0.1], [0.3, 0.3]]])
    z = rng.normal(size=(len(ab), 4)) * 50.0
    raw = np.frombuffer(probe(8, len(ab), 0, ab, z), dtype=np.float64)
    d, x = raw[:len(ab)], raw[len(ab):].reshape(-1, 2)
    assert same_bits(d, S.delta(ab[:, 0], ab[:, 1]))
    assert d[500] == 0.0 and d[501] == 0.0 and d[502] == 0.5 and d[503] == 0.5 and np.isnan(d[504]) and d[505] == 0.0
    assert same_bits(x[:, 0], z[:, 2] * z[:, 0] + z[:, 3] * z[:, 1]) and same_bits(x[:, 1], z[:, 3] * z[:, 0] - z[:, 2] * z[:, 1])
    exact = (z[:, 2] + 1j * z[:, 3]) * np.conj(z[:, 0] + 1j * z[:, 1])
    np.testing.assert_allclose(x[:, 0] + 1j * x[:, 1], exact, rtol=1e-12)
