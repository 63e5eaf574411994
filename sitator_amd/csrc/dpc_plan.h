// Every decision of the density-peak clustering behind SiteTypeAnalysis (site_descriptors/SiteTypeAnalysis.py:99-128, which asks
// pydpc; Rodriguez & Laio, Science 344, 1492 (2014)), written once for the kernels of dpc.hip and for the host compiler
// (tests/test_dpc_plan.py drives it with g++ under ASan / UBSan).  Compile without contraction (-ffp-contract=off): distances are
// compared bit for bit with tests/dpc_ref.py.  Nothing of size N x N is stored: a distance is recomputed wherever it is needed.
//
// Distance.  d(i, j) = sqrt(s_D), s_0 = 0, s_(k+1) = s_k + (y_ik - y_jk) (y_ik - y_jk) for k ascending, every operation rounded on
// its own.  (a - b)^2 and (b - a)^2 are the same bits, so d(i, j) = d(j, i), and it is the same in every kernel.  The kernels
// hold a point in DPp = 2, 4, 8, 16 or 32 registers, the first power of two that takes its D coordinates, the rest zero: a zero
// coordinate adds +0.0 to s, which changes no bit of it.
//
// Kernel size.  dc = the element of rank r = min(floor(0.5 + fraction n), n - 1) (0-based, ascending) among the n = N (N - 1) / 2
// distances d(i, j), i < j.  n and r are 64-bit integers; fraction n is one float64 product (n < 2^53).  Non-negative doubles order
// as their bit patterns taken as unsigned integers, so the element is found by a most-significant-digit radix select on the bit
// pattern: DP_PASSES = 8 passes of DP_DIGIT_BITS = 8 bits.  Pass p counts, per value of bits [56 - 8 p, 64 - 8 p), the distances
// whose bits above those equal the prefix found so far (pass 0: all of them) - 256 unsigned 64-bit counts.  dp_select_step then
// takes the first digit g at which the running total of the counts exceeds r, lowers r by the total below g and appends g to the
// prefix.  After pass 7 the prefix is the bit pattern of dc.  Counts are integers: the result does not depend on who counted what.
//
// Which pairs a workgroup counts.  The points form T = ceil(N / DP_TILE) tiles of DP_TILE.  Block (x, y) of a T x (T / 2 + 1)
// grid takes the tiles a = x and b = (x + y) mod T (dp_tile_pair): every unordered pair of tiles exactly once (for even T the
// blocks y = T / 2 with x >= T / 2 repeat the first half and do nothing).  Thread t holds point i = DP_TILE lo + t in registers,
// the tile hi streams through LDS, and a pair counts when i < j < N.
//
// Density.  rho_i = sum over j != i of w(d(i, j)), w(d) = exp(-(d / dc) (d / dc)) (one division, one product, one negation, one
// exp); for dc = 0 (the rank falls among duplicate points) w(0) = 1 and w(d > 0) = 0, the limit of dc -> 0.  The order of the sum:
// the tiles of j are cut into DP_SPLIT = 8 consecutive segments of ceil(T / 8) tiles; thread i adds the terms of a segment one
// by one in ascending j, starting from 0.0; rho_i = ((((((p_0 + p_1) + p_2) + p_3) + p_4) + p_5) + p_6) + p_7.  No atomics.
//
// Order.  j is ABOVE i iff rho_j > rho_i, or rho_j == rho_i and j < i (dp_above): a total order.  delta_i = the smallest d(i, j)
// over the j above i, neighbour_i its argmin; of equal distances the HIGHEST j in that order wins (dp_better).  A minimum under a
// total order does not depend on the order of the comparisons, so the segments of the density pass are reused.  The top point has
// neighbour -1 and the largest delta of the others.  (pydpc leaves a point whose nearest denser point lies exactly at the
// maximum distance without a neighbour; here it gets that point: DESIGN.md section 18.)
//
// Membership.  Centres: rho_i > min_density and delta_i > min_delta (dp_is_centre), numbered in ascending i.  Every other point
// takes the cluster of its neighbour, transitively; a chain that ends at a point that is no centre and has no neighbour gives -1.
// It is computed by pointer jumping: p_i = i for a centre or a point without neighbour, else neighbour_i; rounds of
// p'_i = p_(p_i) (dp_jump) until nothing changes, at most DP_MAX_ROUNDS of them; membership_i = the number of p_i if it is a
// centre, else -1.
//
// LDS per workgroup: the tile of DP_TILE points of DPp doubles and 2048 bytes (the 256 counts of a select pass, or the densities
// of the tile): 6 144 bytes at DPp = 2, 67 584 at DPp = 32, of the 160 KiB of a gfx950 CU.  All lanes read the same staged point
// at the same time (a broadcast: no bank conflicts).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define DP_HD __host__ __device__
#else
#define DP_HD
#endif

#define DP_BLOCK 256                                   // threads of a workgroup
#define DP_TILE 256                                    // points of a tile: one per thread
#define DP_MAX_D 32                                    // coordinates of a point at most
#define DP_DIGIT_BITS 8
#define DP_PASSES 8
#define DP_BINS 256
#define DP_SPLIT 8                                     // segments of the density and delta sums
#define DP_MAX_N 16777216                              // 2^24 points: 2^16 tiles (the grid), n < 2^47 pairs (64-bit counts, exact in float64)
#define DP_MAX_ABS 1e150                               // |coordinate| the entry point admits: no squared difference overflows
#define DP_MAX_ROUNDS 64                               // pointer jumping: a chain of N <= 2^24 points is done after 25

DP_HD inline int dp_padded(int D) { return D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32; }
DP_HD inline int64_t dp_lds_bytes(int D) { return (int64_t)DP_TILE * dp_padded(D) * 8 + 2048; }
DP_HD inline int64_t dp_tiles(int64_t N) { return (N + DP_TILE - 1) / DP_TILE; }
DP_HD inline int64_t dp_pairs(int64_t N) { return N * (N - 1) / 2; }

// 0: within the limits; otherwise which one is broken (dp_limit_text); invalid_out: the input is wrong rather than too large
inline int dp_check(int64_t N, int64_t D, double fraction, bool *invalid_out)
{
    *invalid_out = true;
    if (N < 2) return 1;
    if (D < 1) return 2;
    if (!(fraction > 0.0 && fraction < 1.0)) return 3;
    *invalid_out = false;
    if (D > DP_MAX_D) return 4;
    if (N > DP_MAX_N) return 5;
    return 0;
}
inline const char *dp_limit_text(int what)
{
    return what == 1 ? "fewer than 2 points" : what == 2 ? "points without coordinates" : what == 3 ? "fraction outside (0, 1)"
         : what == 4 ? "more than 32 coordinates per point (d at most 32)"
         : what == 5 ? "more than 2^24 points (the pair counts of the select are 64-bit integers below 2^47)" : "";
}

template <int DPp> DP_HD inline double dp_dist(const double *a, const double *b)
{
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < DPp; k++) {
        const double t = a[k] - b[k];
        const double q = t * t;
        s = s + q;
    }
    return sqrt(s);
}
// the same for a run-time D (the host)
DP_HD inline double dp_dist_n(const double *a, const double *b, int D)
{
    double s = 0.0;
    for (int k = 0; k < D; k++) {
        const double t = a[k] - b[k];
        const double q = t * t;
        s = s + q;
    }
    return sqrt(s);
}

DP_HD inline uint64_t dp_bits(double d)
{
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
}
DP_HD inline double dp_from_bits(uint64_t u)
{
    double d;
    memcpy(&d, &u, 8);
    return d;
}

DP_HD inline int64_t dp_rank(int64_t n, double fraction)
{
    const int64_t r = (int64_t)floor(0.5 + fraction * (double)n);
    return r < n - 1 ? r : n - 1;
}
// does a distance take part in pass p under the prefix found so far, and with which digit
DP_HD inline bool dp_match(uint64_t bits, int pass, uint64_t prefix)
{
    return pass == 0 || (bits >> (64 - DP_DIGIT_BITS * pass)) == prefix;
}
DP_HD inline int dp_digit(uint64_t bits, int pass)
{
    return (int)((bits >> (64 - DP_DIGIT_BITS * (pass + 1))) & (DP_BINS - 1));
}
// the counts of a pass -> the digit that holds rank *rank; false: the counts hold fewer than *rank + 1 distances
inline bool dp_select_step(const uint64_t hist[DP_BINS], uint64_t *prefix, int64_t *rank)
{
    uint64_t below = 0;
    for (int g = 0; g < DP_BINS; g++) {
        if (below + hist[g] > (uint64_t)*rank) {
            *rank -= (int64_t)below;
            *prefix = (*prefix << DP_DIGIT_BITS) | (uint64_t)g;
            return true;
        }
        below += hist[g];
    }
    return false;
}

// block (x, y) of the T x (T / 2 + 1) grid -> the tiles lo <= hi it takes; false: none
DP_HD inline bool dp_tile_pair(int64_t x, int64_t y, int64_t T, int64_t *lo, int64_t *hi)
{
    if (x >= T || y > T / 2) return false;
    if (T % 2 == 0 && y == T / 2 && y > 0 && x >= T / 2) return false;
    const int64_t b = (x + y) % T;
    *lo = x < b ? x : b;
    *hi = x < b ? b : x;
    return true;
}
// the tiles [first, last) of segment s
DP_HD inline void dp_segment(int64_t T, int s, int64_t *first, int64_t *last)
{
    const int64_t per = (T + DP_SPLIT - 1) / DP_SPLIT;
    const int64_t a = per * s, b = per * (s + 1);
    *first = a < T ? a : T;
    *last = b < T ? b : T;
}

DP_HD inline double dp_weight(double d, double dc)
{
    if (dc > 0.0) {
        const double q = d / dc;
        return exp(-(q * q));
    }
    return d == 0.0 ? 1.0 : 0.0;
}

DP_HD inline bool dp_above(double rho_j, int64_t j, double rho_i, int64_t i)
{
    return rho_j > rho_i || (rho_j == rho_i && j < i);
}
// does the candidate (d, j) replace the incumbent (best_d, best_j; best_j < 0: none)
DP_HD inline bool dp_better(double d, double rho_j, int64_t j, double best_d, double best_rho, int64_t best_j)
{
    if (best_j < 0) return true;
    if (d < best_d) return true;
    return d == best_d && dp_above(rho_j, j, best_rho, best_j);
}

DP_HD inline bool dp_is_centre(double rho, double delta, double min_density, double min_delta)
{
    return rho > min_density && delta > min_delta;
}
// the pointer a point starts with
DP_HD inline int32_t dp_start(int32_t i, bool centre, int32_t neighbour) { return (centre || neighbour < 0) ? i : neighbour; }
