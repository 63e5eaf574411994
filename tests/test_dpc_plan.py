"""CPU-only: the decisions of the density-peak kernels (sitator_amd/csrc/dpc_plan.h) compiled with the host compiler under ASan /
UBSan into a stand-alone probe, the way test_barrier_plan.py builds its own, and driven over stdin / stdout.  Both compilers are
told -ffp-contract=off, so the distance pinned here is the one the kernels evaluate.

The probe walks the pairs the way the kernels do - the grid of tile pairs for the select, the segments of tiles for delta - with
the header's functions, and tests/dpc_ref.py (a dense matrix, a sort, loops) says what must come out: the kernel size bit for bit,
delta bit for bit, neighbour and membership exactly."""
import os
import subprocess

import numpy as np
import pytest

from tests import dpc_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: int64 mode, N, D.
#   mode 0: float64 fraction, Y[N, D]                          -> int64 rank, n; uint64 bits of the kernel size
#   mode 1: float64 Y[N, D], rho[N]                            -> float64 delta[N]; int32 neighbour[N]
#   mode 2: float64 min_density, min_delta, rho[N], delta[N]; int32 neighbour[N] -> int32 membership[N]; int64 rounds
#   mode 3: (N = T)                                            -> int64 visits[T, T] of the tile pairs (lo, hi)
#   mode 4: float64 fraction                                   -> int64 what, invalid
PROBE = r"""
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "dpc_plan.h"

static bool rd(void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, stdin) == n; }
static void wr(const void *p, size_t size, size_t n) { if (n) fwrite(p, size, n, stdout); }

template <int P> static bool padded_agrees(const std::vector<double> &Y, int64_t N, int D)
{
    std::vector<double> Yp((size_t)(N * P), 0.0);
    for (int64_t i = 0; i < N; i++)
        for (int k = 0; k < D; k++) Yp[(size_t)(i * P + k)] = Y[(size_t)(i * D + k)];
    for (int64_t i = 0; i < N; i++)
        for (int64_t j = 0; j < N; j++)
            if (dp_bits(dp_dist<P>(&Yp[(size_t)(i * P)], &Yp[(size_t)(j * P)])) != dp_bits(dp_dist_n(&Y[(size_t)(i * D)], &Y[(size_t)(j * D)], D)))
                return false;
    return true;
}

int main()
{
    int64_t h[3];
    if (fread(h, 8, 3, stdin) != 3) return 2;
    const int64_t mode = h[0], N = h[1];
    const int D = (int)h[2];
    if (N < 0 || N > 100000 || D < 0 || D > 64) return 3;
    if (mode == 0) {
        double fraction;
        std::vector<double> Y((size_t)(N * D));
        if (!rd(&fraction, 8, 1) || !rd(Y.data(), 8, (size_t)(N * D))) return 2;
        bool invalid;
        if (dp_check(N, D, fraction, &invalid)) return 4;
        const int P = dp_padded(D);
        if (!(P == 2 ? padded_agrees<2>(Y, N, D) : P == 4 ? padded_agrees<4>(Y, N, D) : P == 8 ? padded_agrees<8>(Y, N, D)
              : P == 16 ? padded_agrees<16>(Y, N, D) : padded_agrees<32>(Y, N, D))) return 6;
        const int64_t T = dp_tiles(N), n = dp_pairs(N);
        int64_t rank = dp_rank(n, fraction);
        const int64_t rank0 = rank;
        uint64_t prefix = 0;
        for (int pass = 0; pass < DP_PASSES; pass++) {
            uint64_t hist[DP_BINS] = {0};
            for (int64_t x = 0; x < T; x++)
                for (int64_t y = 0; y < T / 2 + 1; y++) {
                    int64_t lo, hi;
                    if (!dp_tile_pair(x, y, T, &lo, &hi)) continue;
                    for (int64_t t = 0; t < DP_TILE; t++)
                        for (int64_t jj = 0; jj < DP_TILE; jj++) {
                            const int64_t i = lo * DP_TILE + t, j = hi * DP_TILE + jj;
                            if (!(i < j && j < N)) continue;
                            const uint64_t bits = dp_bits(dp_dist_n(&Y[(size_t)(i * D)], &Y[(size_t)(j * D)], D));
                            if (dp_match(bits, pass, prefix)) hist[dp_digit(bits, pass)]++;
                        }
                }
            if (!dp_select_step(hist, &prefix, &rank)) return 5;
        }
        const int64_t out[2] = {rank0, n};
        wr(out, 8, 2);
        wr(&prefix, 8, 1);
        return 0;
    }
    if (mode == 1) {
        std::vector<double> Y((size_t)(N * D)), rho((size_t)N), delta((size_t)N, 0.0);
        std::vector<int32_t> nbr((size_t)N, -1);
        if (!rd(Y.data(), 8, (size_t)(N * D)) || !rd(rho.data(), 8, (size_t)N)) return 2;
        const int64_t T = dp_tiles(N);
        int64_t top = -1;
        double largest = 0.0;
        for (int64_t i = 0; i < N; i++) {
            double best_d = 0.0, best_rho = 0.0;
            int64_t best_j = -1;
            for (int s = 0; s < DP_SPLIT; s++) {                 // a segment's own minimum, then the minimum of the segments
                int64_t first, last;
                dp_segment(T, s, &first, &last);
                double sd = 0.0, srho = 0.0;
                int64_t sj = -1;
                for (int64_t j = first * DP_TILE; j < last * DP_TILE && j < N; j++) {
                    if (j == i || !dp_above(rho[(size_t)j], j, rho[(size_t)i], i)) continue;
                    const double d = dp_dist_n(&Y[(size_t)(i * D)], &Y[(size_t)(j * D)], D);
                    if (dp_better(d, rho[(size_t)j], j, sd, srho, sj)) { sd = d; srho = rho[(size_t)j]; sj = j; }
                }
                if (sj >= 0 && dp_better(sd, srho, sj, best_d, best_rho, best_j)) { best_d = sd; best_rho = srho; best_j = sj; }
            }
            nbr[(size_t)i] = (int32_t)best_j;
            delta[(size_t)i] = best_d;
            if (best_j < 0) { if (top >= 0) return 7; top = i; }
            else if (dp_bits(best_d) > dp_bits(largest)) largest = best_d;
        }
        if (top < 0) return 7;
        delta[(size_t)top] = largest;
        wr(delta.data(), 8, (size_t)N);
        wr(nbr.data(), 4, (size_t)N);
        return 0;
    }
    if (mode == 2) {
        double thr[2];
        std::vector<double> rho((size_t)N), delta((size_t)N);
        std::vector<int32_t> nbr((size_t)N), p((size_t)N), q((size_t)N), member((size_t)N), number((size_t)N, -1);
        if (!rd(thr, 8, 2) || !rd(rho.data(), 8, (size_t)N) || !rd(delta.data(), 8, (size_t)N) || !rd(nbr.data(), 4, (size_t)N)) return 2;
        int32_t nc = 0;
        for (int64_t i = 0; i < N; i++) {
            if (nbr[(size_t)i] < -1 || nbr[(size_t)i] >= N) return 3;
            const bool centre = dp_is_centre(rho[(size_t)i], delta[(size_t)i], thr[0], thr[1]);
            if (centre) number[(size_t)i] = nc++;
            p[(size_t)i] = dp_start((int32_t)i, centre, nbr[(size_t)i]);
        }
        int64_t rounds = 0;
        for (bool changed = true; changed && rounds < DP_MAX_ROUNDS; rounds++) {
            changed = false;
            for (int64_t i = 0; i < N; i++) {
                q[(size_t)i] = p[(size_t)p[(size_t)i]];
                changed = changed || q[(size_t)i] != p[(size_t)i];
            }
            p.swap(q);
        }
        for (int64_t i = 0; i < N; i++) member[(size_t)i] = number[(size_t)p[(size_t)i]];
        wr(member.data(), 4, (size_t)N);
        wr(&rounds, 8, 1);
        return 0;
    }
    if (mode == 3) {
        const int64_t T = N;
        std::vector<int64_t> visits((size_t)(T * T), 0);
        for (int64_t x = 0; x < T + 2; x++)
            for (int64_t y = 0; y < T / 2 + 3; y++) {
                int64_t lo = -1, hi = -1;
                if (!dp_tile_pair(x, y, T, &lo, &hi)) continue;
                if (lo < 0 || hi >= T || lo > hi) return 8;
                visits[(size_t)(lo * T + hi)]++;
            }
        wr(visits.data(), 8, (size_t)(T * T));
        return 0;
    }
    if (mode == 4) {
        double fraction;
        if (!rd(&fraction, 8, 1)) return 2;
        bool invalid = false;
        const int64_t out[2] = {dp_check(N, h[2], fraction, &invalid), invalid ? 1 : 0};
        wr(out, 8, 2);
        if (out[0] && !dp_limit_text((int)out[0])[0]) return 9;
        return 0;
    }
    return 3;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    td = tmp_path_factory.mktemp("dpc_plan")
    src = td / "probe.cpp"
    src.write_text(PROBE)
    exe = str(td / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sitator_amd", "csrc"), str(src), "-o", exe])

    def run(mode, N, D, *arrays):
        data = np.array([mode, N, D], dtype=np.int64).tobytes() + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
        return subprocess.run([exe], input=data, stdout=subprocess.PIPE, check=True).stdout
    return run


def f64(*values):
    return np.array(values, dtype=np.float64)


def select(probe, Y, fraction):
    raw = probe(0, Y.shape[0], Y.shape[1], f64(fraction), Y.astype(np.float64))
    rank, n = np.frombuffer(raw[:16], dtype=np.int64)
    return np.frombuffer(raw[16:24], dtype=np.uint64)[0], int(rank), int(n)


def cloud(N, D, seed):
    return np.random.default_rng(seed).normal(size=(N, D))


def last_digit_points():
    """Points on a line whose pairwise distances are 1 + k 2^-52, k = 0..: equal in every digit but the last of the last pass."""
    x = np.array([0.0] + [1.0 + k * 2.0 ** -52 for k in range(40)])
    return x[:, None]


SELECT_CASES = {
    "cloud_d2": (cloud(40, 2, 1), [1e-9, 0.02, 0.5, 0.999, 1.0 - 1e-12]),
    "cloud_d5_two_tiles": (cloud(300, 5, 2), [1e-9, 0.02, 0.9999999]),
    "two_points": (cloud(2, 3, 3), [0.01, 0.5, 0.99]),
    "three_points": (cloud(3, 1, 4), [0.1, 0.5, 0.9]),
    "all_equal": (np.ones((17, 3)) * 0.37, [0.02, 0.5]),
    "duplicates": (np.repeat(cloud(6, 2, 5), 5, axis=0), [1e-9, 0.05, 0.12, 0.5]),
    "last_digit": (last_digit_points(), [1e-9, 0.953, 0.96, 0.97, 0.98, 0.99, 0.999]),      # ranks 780.. are the 40 distances from point 0
    "cap_d32": (cloud(20, 32, 6), [0.02, 0.5]),
}


@pytest.mark.parametrize("name", sorted(SELECT_CASES))
def test_radix_select_is_the_sorted_element(probe, name):
    Y, fractions = SELECT_CASES[name]
    dist = DR.distances(Y)
    seen = set()
    for fraction in fractions:
        dc, rank, n = DR.kernel_size(dist, fraction)
        bits, got_rank, got_n = select(probe, Y, fraction)
        assert (got_rank, got_n) == (rank, n)
        assert bits == np.float64(dc).view(np.uint64), "%s at %r: the select gave %r, the sort %r" % (
            name, fraction, np.uint64(bits).view(np.float64), dc)
        seen.add(rank)
    if name == "cloud_d2":
        n = 40 * 39 // 2
        assert 0 in seen and n - 1 in seen
        assert DR.rank_of(n, 1.0 - 1e-12) == n - 1 and int(np.floor(0.5 + (1.0 - 1e-12) * n)) == n     # the clamp cuts this one
    if name == "duplicates":
        assert DR.kernel_size(dist, 0.05)[0] == 0.0 and DR.kernel_size(dist, 0.5)[0] > 0.0
    if name == "last_digit":
        firsts = np.sort(dist[0, 1:])
        assert np.all(np.diff(firsts.view(np.uint64)) == 1)          # neighbours in the last bit
        sizes = [np.float64(DR.kernel_size(dist, f)[0]).view(np.uint64) for f in fractions[1:]]
        assert len(set(int(s) >> 8 for s in sizes)) == 1 and len(set(int(s) for s in sizes)) == len(sizes)


def graph_inputs():
    rng = np.random.default_rng(11)
    blob = np.concatenate([rng.normal(size=(30, 2)) * 0.3, rng.normal(size=(30, 2)) * 0.3 + [4.0, 0.0]])
    dup = np.concatenate([blob[:10], blob[:10], blob[:10], blob[40:45]])              # equal densities, zero distances
    square = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [3.0, 3.0]])     # equal distances to denser points
    return {"blobs": blob, "duplicates": dup, "square": square, "tiles": rng.normal(size=(600, 3))}


@pytest.mark.parametrize("name", ["blobs", "duplicates", "square", "tiles"])
def test_delta_and_neighbour_follow_the_tie_rules(probe, name):
    Y = graph_inputs()[name]
    dist = DR.distances(Y)
    dc = DR.kernel_size(dist, 0.1)[0]
    rho = DR.density(dist, dc)
    if name == "square":
        rho = np.array([1.0, 3.0, 3.0, 2.0, 3.0, 0.5])              # 0 is equally far from 1, 2 and 4 (equal densities): 1 is highest
    if name == "duplicates":
        rho[10:20] = rho[20:30] = rho[:10]                          # numpy's row sums of equal rows may differ in the last bit
        assert len(np.unique(rho[:30])) <= 10 and np.sum(dist == 0.0) > len(Y)
    delta, nbr = DR.delta_neighbour(dist, rho)
    raw = probe(1, Y.shape[0], Y.shape[1], Y.astype(np.float64), rho)
    N = len(Y)
    got_delta = np.frombuffer(raw[:8 * N], dtype=np.float64)
    got_nbr = np.frombuffer(raw[8 * N:], dtype=np.int32)
    assert np.array_equal(got_nbr, nbr)
    assert np.array_equal(got_delta.view(np.uint64), delta.view(np.uint64))
    if name == "square":
        assert nbr[0] == 1 and nbr[3] == 2 and nbr[5] == 1 and nbr[1] == -1
    if name == "duplicates":
        assert np.sum(delta == 0.0) >= 20                            # a duplicate's nearest point above is its twin


def test_membership_with_a_chain_that_ends_nowhere(probe):
    #        0 <- 1 <- 2      3 <- 4 (3: no centre, no neighbour)      5 a centre on its own, 6 -> 5
    rho = np.array([9.0, 5.0, 4.0, 0.1, 0.05, 8.0, 3.0])
    delta = np.array([7.0, 0.5, 0.4, 6.0, 0.3, 6.5, 0.2])
    nbr = np.array([-1, 0, 1, -1, 3, 0, 5], dtype=np.int32)
    for thr in [(1.0, 1.0), (0.0, 5.0), (8.5, 1.0), (100.0, 100.0)]:
        member, clusters = DR.assign(rho, delta, nbr, *thr)
        raw = probe(2, len(rho), 1, f64(*thr), rho, delta, nbr)
        got = np.frombuffer(raw[:4 * len(rho)], dtype=np.int32)
        assert np.array_equal(got, member), thr
    member, clusters = DR.assign(rho, delta, nbr, 1.0, 1.0)
    assert list(clusters) == [0, 5] and list(member) == [0, 0, 0, -1, -1, 1, 1]
    # a long chain: as many rounds as its length has bits, not as it has links
    N = 1000
    rho, delta, nbr = np.arange(N, 0, -1.0), np.ones(N), np.arange(-1, N - 1, dtype=np.int32)
    delta[0] = 5.0
    raw = probe(2, N, 1, f64(0.0, 2.0), rho, delta, nbr)
    assert np.all(np.frombuffer(raw[:4 * N], dtype=np.int32) == 0)
    assert np.frombuffer(raw[4 * N:], dtype=np.int64)[0] <= 11


@pytest.mark.parametrize("T", list(range(1, 10)))
def test_every_pair_of_tiles_is_taken_once(probe, T):
    visits = np.frombuffer(probe(3, T, 0), dtype=np.int64).reshape(T, T)
    assert np.array_equal(visits, np.triu(np.ones((T, T), dtype=np.int64)))


def test_limits(probe):
    def check(N, D, fraction):
        return tuple(np.frombuffer(probe(4, N, D, f64(fraction)), dtype=np.int64))
    assert check(2, 1, 0.5) == (0, 0) and check(100000, 32, 0.02) == (0, 0)
    assert check(1, 2, 0.5) == (1, 1) and check(5, 0, 0.5) == (2, 1)
    for fraction in (0.0, 1.0, -0.1, np.nan, np.inf):
        assert check(5, 2, fraction) == (3, 1)
    assert check(5, 33, 0.5) == (4, 0)
