// Every decision of DensityPercolation (percolation.hip), in ONE place: the neighbour and the shift of a voxel under an offset,
// which edges a labelling round and the seam pass look at, the hook and compress rules (those of pathway_graph.h) and a serial
// driver of them, the quotient step - a union-find with integer offsets over the seam records and a Hermite normal form per
// component - the bisection over the bit patterns of the positive doubles and its snap rule, the limits, the plan and - pc_layout(),
// the one place that names them - the pieces of a call's device buffer.  Host and device integer arithmetic only: no HIP call, no
// context, no side effect (tests/test_percolation_plan.py compiles it with g++ under ASan / UBSan).
//
// Definitions.  Grid n = (n0, n1, n2), V = n0 n1 n2, flat index v = (i0 n1 + i1) n2 + i2:
//   offsets   d in {-1, 0, 1}^3 with 1 (connectivity 6), at most 2 (18) or at most 3 (26) non-zero entries; offset k = 9 (d0 + 1)
//             + 3 (d1 + 1) + (d2 + 1), k = 13 is no offset, k > 13 the lexicographically positive half
//   edge      the neighbour of i under d is (i + d) mod n, with the shift s_a = floor((i_a + d_a) / n_a) in {-1, 0, 1}; s = 0: an
//             INTERIOR edge, else a SEAM edge.  The shift code is 9 (s0 + 1) + 3 (s1 + 1) + (s2 + 1), 13 for s = 0.  Every
//             undirected edge is looked at once: an interior one from its end with the positive offset (k > 13), a seam one from
//             the end that sees the positive shift (code > 13)
//   set       the voxels with g[v] >= level (a NaN never passes); label[v] = the lowest flat index of v's component, -1 outside
//   lattice   the shift sums around the closed walks of a component generate L in Z^3; rank = rank L, basis = the row Hermite
//             normal form of L (upper triangular, positive pivots, entries above a pivot in [0, pivot), zero rows last)
//   levels    t_d = the largest positive value of g at which the set has a component of rank >= d, 0.0 if {g > 0} has none
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "scratch_carve.h"
#include "pathway_graph.h"

#define PC_HD CP_HD inline

#define PC_THREADS 256                            // threads of a workgroup of every kernel: four waves
#define PC_MAX_GRID 1024                          // voxels along an axis, as density_plan.h
#define PC_MAX_VOXELS ((int64_t)1 << 27)          // a label is an int32, a seam count a uint32
#define PC_TILE0 8                                // the tile of the local phase: 8 x 8 x 16 voxels, four per thread, the last axis
#define PC_TILE1 8                                // across lanes; its labels are 4 KB of LDS
#define PC_TILE2 16
#define PC_TILE_VOXELS (PC_TILE0 * PC_TILE1 * PC_TILE2)
#define PC_PER_THREAD (PC_TILE_VOXELS / PC_THREADS)
#define PC_FORM_GLOBAL 1                          // global rounds from label[v] = v
#define PC_FORM_TILE 2                            // a tile-local fixed point in LDS first; global rounds look at edges between tiles only
#define PC_NO_OFFSET 13
#define PC_RECORD_WORDS 12                        // a component record: root, size, rank, basis[9]
#define PC_WORDS 16                               // u64 words of a call: {change flag, seam cursor, min bits, max bits, ..}

// ---- offsets, neighbours, shifts ------------------------------------------------------------------------------------------

PC_HD bool pc_connectivity_ok(int conn) { return conn == 6 || conn == 18 || conn == 26; }

PC_HD void pc_offset(int k, int *d) { d[0] = k / 9 - 1; d[1] = k / 3 % 3 - 1; d[2] = k % 3 - 1; }

// offset k belongs to the connectivity
PC_HD bool pc_offset_in(int conn, int k)
{
    int d[3];
    pc_offset(k, d);
    const int nz = (d[0] != 0) + (d[1] != 0) + (d[2] != 0);
    return nz >= 1 && nz <= (conn == 6 ? 1 : conn == 18 ? 2 : 3);
}

// the neighbour j of index i (in [0, n)) under d (in {-1, 0, 1}) along an axis of n voxels and the shift floor((i + d) / n)
PC_HD void pc_neighbour(int64_t i, int d, int64_t n, int64_t *j, int *s)
{
    const int64_t t = i + d;
    *s = t < 0 ? -1 : (t >= n ? 1 : 0);
    *j = t - (int64_t)*s * n;
}

PC_HD int pc_shift_code(const int *s) { return 9 * (s[0] + 1) + 3 * (s[1] + 1) + (s[2] + 1); }

PC_HD void pc_coords(int64_t v, const int64_t *n, int64_t *i)
{
    i[2] = v % n[2]; i[1] = (v / n[2]) % n[1]; i[0] = v / (n[1] * n[2]);
}

// the edge of voxel i under offset k: the neighbour's flat index and the shift code
PC_HD int64_t pc_edge(const int64_t *i, const int64_t *n, int k, int *code)
{
    int d[3], s[3];
    int64_t j[3];
    pc_offset(k, d);
    for (int a = 0; a < 3; a++) pc_neighbour(i[a], d[a], n[a], &j[a], &s[a]);
    *code = pc_shift_code(s);
    return (j[0] * n[1] + j[1]) * n[2] + j[2];
}

// a labelling round looks at this edge (from this end)
PC_HD bool pc_is_interior_forward(int k, int code) { return k > PC_NO_OFFSET && code == PC_NO_OFFSET; }
// the seam pass records this edge (from this end)
PC_HD bool pc_is_seam_forward(int code) { return code > PC_NO_OFFSET; }

PC_HD bool pc_in_set(double g, double level) { return g >= level; }          // a NaN never passes

PC_HD int64_t pc_tile_of(const int64_t *i, const int64_t *tiles)
{
    return ((i[0] / PC_TILE0) * tiles[1] + i[1] / PC_TILE1) * tiles[2] + i[2] / PC_TILE2;
}

// ---- the bit patterns of the positive doubles ---------------------------------------------------------------------------------

PC_HD uint64_t pc_bits(double g) { uint64_t b; memcpy(&b, &g, 8); return b; }
PC_HD double pc_value(uint64_t b) { double g; memcpy(&g, &b, 8); return g; }
// g is a candidate of the reduction above `lo_bits`: positive (a NaN is not) and, as a bit pattern, at least lo_bits - for positive
// doubles the order of the patterns is the order of the values.  The snap of a level is the smallest candidate's pattern
PC_HD bool pc_candidate(double g, uint64_t lo_bits) { return g > 0.0 && pc_bits(g) >= lo_bits; }

// The three searches over one bracket table.  known_true[d] (0: none yet) is the largest pattern known to have a component of rank > d
// in its set, known_false[d] the smallest known to have none (one past the maximum to begin with: an empty set).  A probe at `bits`
// comes with its snaps - `above`, the smallest pattern of a positive value at or above bits, and `below`, the largest one under it (0:
// none): every level in (below, above] has the set of the probe, so a probe moves a bracket to a value of the grid, and all three
// brackets at once.  Search d is over when the two meet, or when the smallest positive value itself has no such component
struct PcSearch {
    uint64_t min_bits, max_bits;                  // of the positive values; min_bits == 0: there is none
    uint64_t known_true[3], known_false[3];
    int rank_at[3];                               // the largest rank at known_true
};

inline void pc_search_init(PcSearch &s, uint64_t min_bits, uint64_t max_bits)
{
    s.min_bits = min_bits; s.max_bits = max_bits;
    for (int d = 0; d < 3; d++) { s.known_true[d] = 0; s.known_false[d] = max_bits + 1; s.rank_at[d] = 0; }
}

// the next pattern to probe, false when every search is over
inline bool pc_search_next(const PcSearch &s, uint64_t *bits)
{
    if (s.min_bits == 0) return false;
    for (int d = 0; d < 3; d++) {
        if (s.known_true[d] == 0) {
            if (s.known_false[d] <= s.min_bits) continue;                       // t_d = 0
            *bits = s.min_bits;
            return true;
        }
        if (s.known_true[d] + 1 >= s.known_false[d]) continue;
        *bits = s.known_true[d] + (s.known_false[d] - s.known_true[d]) / 2;     // strictly between the two
        return true;
    }
    return false;
}

inline void pc_search_update(PcSearch &s, int rank, uint64_t above, uint64_t below)
{
    for (int d = 0; d < 3; d++) {
        if (rank > d) { if (above > s.known_true[d]) { s.known_true[d] = above; s.rank_at[d] = rank; } }
        else if (below + 1 < s.known_false[d]) s.known_false[d] = below + 1;
    }
}

// ---- the Hermite normal form ----------------------------------------------------------------------------------------------

typedef __int128 pc_wide;

// row[c] is the row whose pivot is column c (row[c][c] > 0), all zero where the lattice has none.  Kept canonical between calls
struct PcLattice {
    pc_wide row[3][3];
    int rank;
};

inline void pc_lattice_clear(PcLattice &L) { memset(&L, 0, sizeof(L)); }
inline bool pc_lattice_full(const PcLattice &L) { return L.rank == 3 && L.row[0][0] == 1 && L.row[1][1] == 1 && L.row[2][2] == 1; }

// Two integer types run the one insertion below.  PcI128: 127 bits and a flag that an operation left them - what every shift sum
// needs, and fast.  PcBig: 511 bits in sign and magnitude, taken only when the first gave up: the normal form of generators of 31
// bits has entries below the determinant (2^96), but the row Euclid that finds it multiplies rows of about 2^62 by quotients of
// about 2^62 before they cancel, and an entry of a column without a pivot has nothing to be reduced by
struct PcI128 {
    pc_wide v;
    bool bad;
    static PcI128 from(pc_wide x) { PcI128 r; r.v = x; r.bad = false; return r; }
    bool to(pc_wide *x) const { *x = v; return !bad; }
    bool is_zero() const { return v == 0; }
    bool is_neg() const { return v < 0; }
};
inline PcI128 operator-(const PcI128 &a, const PcI128 &b) { PcI128 r; r.bad = __builtin_sub_overflow(a.v, b.v, &r.v) || a.bad || b.bad; return r; }
inline PcI128 operator*(const PcI128 &a, const PcI128 &b) { PcI128 r; r.bad = __builtin_mul_overflow(a.v, b.v, &r.v) || a.bad || b.bad; return r; }
inline PcI128 operator-(const PcI128 &a) { return PcI128::from(0) - a; }
inline PcI128 operator/(const PcI128 &a, const PcI128 &b)                       // truncated; the one quotient that overflows is -2^127 / -1
{
    PcI128 r;
    r.bad = a.bad || b.bad || b.v == 0 || (b.v == -1 && (unsigned __int128)a.v == ((unsigned __int128)1 << 127));
    r.v = r.bad ? 0 : a.v / b.v;
    return r;
}
inline PcI128 operator%(const PcI128 &a, const PcI128 &b)
{
    PcI128 r;
    r.bad = a.bad || b.bad || b.v == 0;
    r.v = (r.bad || b.v == -1) ? 0 : a.v % b.v;
    return r;
}

#define PC_BIG_LIMBS 8
struct PcBig {
    uint64_t m[PC_BIG_LIMBS];                     // the magnitude, lowest limb first
    bool neg, bad;
    static PcBig from(pc_wide x)
    {
        PcBig r;
        memset(&r, 0, sizeof(r));
        r.neg = x < 0;
        const unsigned __int128 u = x < 0 ? (unsigned __int128)0 - (unsigned __int128)x : (unsigned __int128)x;
        r.m[0] = (uint64_t)u; r.m[1] = (uint64_t)(u >> 64);
        return r;
    }
    bool to(pc_wide *x) const
    {
        for (int i = 2; i < PC_BIG_LIMBS; i++)
            if (m[i]) return false;
        if (bad || (m[1] >> 63)) return false;
        const pc_wide u = (pc_wide)(((unsigned __int128)m[1] << 64) | m[0]);
        *x = neg ? -u : u;
        return true;
    }
    bool is_zero() const
    {
        for (int i = 0; i < PC_BIG_LIMBS; i++)
            if (m[i]) return false;
        return true;
    }
    bool is_neg() const { return neg && !is_zero(); }
};
inline int pc_mag_cmp(const PcBig &a, const PcBig &b)
{
    for (int i = PC_BIG_LIMBS - 1; i >= 0; i--)
        if (a.m[i] != b.m[i]) return a.m[i] < b.m[i] ? -1 : 1;
    return 0;
}
// r = |a| + |b| (true: a carry left the limbs) and r = |a| - |b| for |a| >= |b|
inline bool pc_mag_add(PcBig &r, const PcBig &a, const PcBig &b)
{
    unsigned __int128 carry = 0;
    for (int i = 0; i < PC_BIG_LIMBS; i++) { carry += (unsigned __int128)a.m[i] + b.m[i]; r.m[i] = (uint64_t)carry; carry >>= 64; }
    return carry != 0;
}
inline void pc_mag_sub(PcBig &r, const PcBig &a, const PcBig &b)
{
    uint64_t borrow = 0;
    for (int i = 0; i < PC_BIG_LIMBS; i++) {
        const uint64_t x = a.m[i], y = b.m[i], d = x - y - borrow;
        borrow = (x < y || (x == y && borrow)) ? 1 : 0;
        r.m[i] = d;
    }
}
inline PcBig operator-(const PcBig &a) { PcBig r = a; r.neg = !a.neg; return r; }
inline PcBig operator-(const PcBig &a, const PcBig &b)
{
    PcBig r;
    memset(&r, 0, sizeof(r));
    r.bad = a.bad || b.bad;
    const bool b_neg = !b.neg;                                                  // a + (-b)
    if (a.neg == b_neg) { r.neg = a.neg; r.bad = pc_mag_add(r, a, b) || r.bad; }
    else if (pc_mag_cmp(a, b) >= 0) { r.neg = a.neg; pc_mag_sub(r, a, b); }
    else { r.neg = b_neg; pc_mag_sub(r, b, a); }
    return r;
}
inline PcBig operator*(const PcBig &a, const PcBig &b)
{
    PcBig r;
    memset(&r, 0, sizeof(r));
    r.bad = a.bad || b.bad;
    r.neg = a.neg != b.neg;
    for (int i = 0; i < PC_BIG_LIMBS; i++) {
        if (!a.m[i]) continue;
        unsigned __int128 carry = 0;
        for (int j = 0; j < PC_BIG_LIMBS; j++) {
            if (i + j >= PC_BIG_LIMBS) { if (b.m[j]) r.bad = true; continue; }
            carry += (unsigned __int128)a.m[i] * b.m[j] + r.m[i + j];
            r.m[i + j] = (uint64_t)carry;
            carry >>= 64;
        }
        if (carry) r.bad = true;
    }
    return r;
}
// |a| = q |b| + rem, bit by bit from the highest set bit of |a|
inline void pc_mag_divmod(const PcBig &a, const PcBig &b, PcBig &q, PcBig &rem)
{
    memset(&q, 0, sizeof(q));
    memset(&rem, 0, sizeof(rem));
    if (b.is_zero()) { q.bad = rem.bad = true; return; }
    for (int bit = 64 * PC_BIG_LIMBS - 1; bit >= 0; bit--) {
        if (rem.m[PC_BIG_LIMBS - 1] >> 63) { q.bad = rem.bad = true; return; }
        for (int i = PC_BIG_LIMBS - 1; i > 0; i--) rem.m[i] = (rem.m[i] << 1) | (rem.m[i - 1] >> 63);
        rem.m[0] = (rem.m[0] << 1) | ((a.m[bit / 64] >> (bit % 64)) & 1);
        if (pc_mag_cmp(rem, b) >= 0) { pc_mag_sub(rem, rem, b); q.m[bit / 64] |= (uint64_t)1 << (bit % 64); }
    }
}
inline PcBig operator/(const PcBig &a, const PcBig &b)                          // truncated
{
    PcBig q, rem;
    pc_mag_divmod(a, b, q, rem);
    q.neg = a.neg != b.neg;
    q.bad = q.bad || a.bad || b.bad;
    return q;
}
inline PcBig operator%(const PcBig &a, const PcBig &b)                          // the sign of a, as the built-in
{
    PcBig q, rem;
    pc_mag_divmod(a, b, q, rem);
    rem.neg = a.neg;
    rem.bad = rem.bad || a.bad || b.bad;
    return rem;
}

template <class I> inline I pc_floor_div(const I &a, const I &b)                // b > 0
{
    const I q = a / b;
    return (!(a % b).is_zero() && a.is_neg()) ? q - I::from(1) : q;
}

// r -= q * p over the columns from c on
template <class I> inline void pc_row_sub(I *r, const I &q, const I *p, int c)
{
    for (int k = c; k < 3; k++) r[k] = r[k] - q * p[k];
}

// the entries of r in the pivot columns beyond c into [0, pivot): the columns in ascending order, a row changes only what lies behind its pivot
template <class I> inline void pc_reduce_tail(I (*row)[3], I *r, int c)
{
    for (int k = c + 1; k < 3; k++)
        if (!row[k][k].is_zero()) pc_row_sub(r, pc_floor_div(r[k], row[k][k]), row[k], k);
}

// rows += Z v, canonical again; false: an operation left the type
template <class I> inline bool pc_hnf_insert_rows(I (*row)[3], const pc_wide *v_in)
{
    I v[3] = {I::from(v_in[0]), I::from(v_in[1]), I::from(v_in[2])};
    for (int c = 0; c < 3; c++) {
        pc_reduce_tail(row, v, c);                                              // keeps what follows small
        if (v[c].is_zero()) continue;
        I *p = row[c];
        while (!v[c].is_zero()) {                                               // Euclid on column c between the pivot row and v
            if (v[c].bad || p[c].bad) return false;
            if (!p[c].is_zero()) {
                pc_row_sub(p, p[c] / v[c], v, c);
                pc_reduce_tail(row, p, c);
            }
            for (int k = 0; k < 3; k++) { const I t = p[k]; p[k] = v[k]; v[k] = t; }
        }
        if (p[c].is_neg())
            for (int k = c; k < 3; k++) p[k] = -p[k];
        pc_reduce_tail(row, p, c);
    }
    for (int c = 0; c < 3; c++)                                                 // a new or smaller pivot: the rows above it again
        if (!row[c][c].is_zero()) pc_reduce_tail(row, row[c], c);
    for (int i = 0; i < 9; i++)
        if (row[i / 3][i % 3].bad) return false;
    return true;
}

template <class I> inline bool pc_hnf_insert_as(PcLattice &L, const pc_wide *v)
{
    I row[3][3];
    pc_wide out[3][3];
    for (int i = 0; i < 9; i++) row[i / 3][i % 3] = I::from(L.row[i / 3][i % 3]);
    if (!pc_hnf_insert_rows(row, v)) return false;
    for (int i = 0; i < 9; i++)
        if (!row[i / 3][i % 3].to(&out[i / 3][i % 3])) return false;
    memcpy(L.row, out, sizeof(out));
    L.rank = (L.row[0][0] != 0) + (L.row[1][1] != 0) + (L.row[2][2] != 0);
    return true;
}

// L += Z v.  false (L as it was): an entry of the normal form itself does not fit 127 bits, or an intermediate left 511 - neither
// for generators of 32 bits or fewer
inline bool pc_hnf_insert(PcLattice &L, const pc_wide *v)
{
    return pc_hnf_insert_as<PcI128>(L, v) || pc_hnf_insert_as<PcBig>(L, v);
}

// the canonical form: the pivot rows in column order, zero rows last
inline void pc_lattice_rows(const PcLattice &L, pc_wide out[3][3])
{
    int r = 0;
    memset(out, 0, 9 * sizeof(pc_wide));
    for (int c = 0; c < 3; c++)
        if (L.row[c][c] != 0) { for (int k = 0; k < 3; k++) out[r][k] = L.row[c][k]; r++; }
}

// ... as int32; false where an entry does not fit
inline bool pc_lattice_basis(const PcLattice &L, int32_t *basis9)
{
    pc_wide rows[3][3];
    pc_lattice_rows(L, rows);
    for (int i = 0; i < 9; i++) {
        const pc_wide x = rows[i / 3][i % 3];
        if (x < INT32_MIN || x > INT32_MAX) return false;
        basis9[i] = (int32_t)x;
    }
    return true;
}

// ---- the quotient step ------------------------------------------------------------------------------------------------------

struct PcComponent { int32_t root, rank, basis[9]; };

struct PcQuotient {
    std::vector<int32_t> pairs;                   // (open root, periodic root) for every open root that is not its component's lowest
    std::vector<PcComponent> comps;               // the components of rank > 0, by ascending root
    int max_rank;
    int64_t cycles, distinct;                     // records that closed a cycle with a non-zero shift sum; distinct records
};

// The open components are nodes, a seam record (label_u, label_v, code) an edge whose far end lies s = code's shift further:
// potential(v) = potential(u) + s.  A union-find keeps for every node its potential relative to its parent; the lower root becomes
// the parent, so a class's root is its lowest open root - the periodic label.  A record inside a class closes a cycle: its shift sum
// goes into the class's lattice (and the lattices of two classes that meet are added).  first_full_ends: the caller asks for the largest
// rank only, and the call ends at the first lattice that is Z^3.  false: a label below 0, a code that is no shift, or an overflow
inline bool pc_quotient(const int32_t *rec, int64_t n_rec, bool first_full_ends, PcQuotient &out)
{
    out.pairs.clear(); out.comps.clear();
    out.max_rank = 0; out.cycles = 0; out.distinct = 0;
    std::unordered_map<int32_t, int32_t> id;
    std::unordered_set<uint64_t> seen;
    std::vector<int32_t> value, parent, lat_of;
    std::vector<int64_t> off;                     // [node][3]
    std::vector<PcLattice> lats;
    auto node = [&](int32_t label) {
        auto it = id.find(label);
        if (it != id.end()) return it->second;
        const int32_t x = (int32_t)value.size();
        id.emplace(label, x);
        value.push_back(label); parent.push_back(x); lat_of.push_back(-1);
        off.push_back(0); off.push_back(0); off.push_back(0);
        return x;
    };
    auto find = [&](int32_t x, int64_t *pot) {
        int64_t sum[3] = {0, 0, 0};
        int32_t r = x;
        while (parent[r] != r) { for (int a = 0; a < 3; a++) sum[a] += off[3 * (size_t)r + a]; r = parent[r]; }
        int64_t acc[3] = {sum[0], sum[1], sum[2]};
        for (int32_t cur = x; parent[cur] != cur;) {
            const int32_t next = parent[cur];
            for (int a = 0; a < 3; a++) { const int64_t o = off[3 * (size_t)cur + a]; off[3 * (size_t)cur + a] = acc[a]; acc[a] -= o; }
            parent[cur] = r;
            cur = next;
        }
        for (int a = 0; a < 3; a++) pot[a] = sum[a];
        return r;
    };
    bool done = false;
    for (int64_t e = 0; e < n_rec && !done; e++) {
        const int32_t lu = rec[3 * e], lv = rec[3 * e + 1], code = rec[3 * e + 2];
        if (lu < 0 || lv < 0 || code < 0 || code > 26 || code == PC_NO_OFFSET) return false;
        if (!seen.insert(((uint64_t)(uint32_t)lu << 32) | ((uint64_t)(uint32_t)lv << 5) | (uint64_t)code).second) continue;
        out.distinct++;
        const int64_t s[3] = {code / 9 - 1, code / 3 % 3 - 1, code % 3 - 1};
        int64_t pu[3], pv[3];
        const int32_t ru = find(node(lu), pu), rv = find(node(lv), pv);
        if (ru != rv) {
            const bool u_stays = value[ru] < value[rv];
            const int32_t top = u_stays ? ru : rv, sub = u_stays ? rv : ru;
            // potential(sub's root) - potential(top's root), from potential(v) = potential(u) + s
            for (int a = 0; a < 3; a++) off[3 * (size_t)sub + a] = u_stays ? pu[a] + s[a] - pv[a] : pv[a] - s[a] - pu[a];
            parent[sub] = top;
            if (lat_of[sub] >= 0) {
                if (lat_of[top] < 0) lat_of[top] = lat_of[sub];
                else {
                    PcLattice &L = lats[(size_t)lat_of[top]];
                    const PcLattice &S = lats[(size_t)lat_of[sub]];
                    for (int c = 0; c < 3; c++)
                        if (S.row[c][c] != 0 && !pc_lattice_full(L) && !pc_hnf_insert(L, S.row[c])) return false;
                    if (L.rank > out.max_rank) out.max_rank = L.rank;
                }
            }
            continue;
        }
        const pc_wide loop[3] = {(pc_wide)(pu[0] + s[0] - pv[0]), (pc_wide)(pu[1] + s[1] - pv[1]), (pc_wide)(pu[2] + s[2] - pv[2])};
        if (loop[0] == 0 && loop[1] == 0 && loop[2] == 0) continue;
        out.cycles++;
        if (lat_of[ru] < 0) {
            lat_of[ru] = (int32_t)lats.size();
            lats.push_back(PcLattice());
            pc_lattice_clear(lats.back());
        }
        PcLattice &L = lats[(size_t)lat_of[ru]];
        if (pc_lattice_full(L)) continue;
        if (!pc_hnf_insert(L, loop)) return false;
        if (L.rank > out.max_rank) out.max_rank = L.rank;
        if (first_full_ends && pc_lattice_full(L)) done = true;
    }
    if (first_full_ends) return true;
    int64_t pot[3];
    for (int32_t x = 0; x < (int32_t)value.size(); x++) {
        const int32_t r = find(x, pot);
        if (r != x) { out.pairs.push_back(value[x]); out.pairs.push_back(value[r]); continue; }
        if (lat_of[x] < 0) continue;
        PcComponent comp;
        comp.root = value[x]; comp.rank = lats[(size_t)lat_of[x]].rank;
        if (!pc_lattice_basis(lats[(size_t)lat_of[x]], comp.basis)) return false;
        out.comps.push_back(comp);
    }
    std::sort(out.comps.begin(), out.comps.end(), [](const PcComponent &a, const PcComponent &b) { return a.root < b.root; });
    return true;
}

// ---- a serial driver of the same rules ----------------------------------------------------------------------------------------

// label[v] = v in the set, -1 outside
inline void pc_init_serial(const double *grid, int64_t V, double level, int32_t *label)
{
    for (int64_t v = 0; v < V; v++) label[v] = pc_in_set(grid[v], level) ? (int32_t)v : -1;
}

// rounds of hook over every interior edge and compress over every voxel until a hook pass finds equal labels everywhere;
// tile_first: the edges inside a tile are brought to their fixed point first (tile by tile), the rounds then look at the others,
// and a last one at all of them
inline int64_t pc_label_serial(const int64_t *n, int conn, bool tile_first, int32_t *label)
{
    const int64_t V = n[0] * n[1] * n[2];
    const int64_t tiles[3] = {(n[0] + PC_TILE0 - 1) / PC_TILE0, (n[1] + PC_TILE1 - 1) / PC_TILE1, (n[2] + PC_TILE2 - 1) / PC_TILE2};
    auto get = [&](int x) { return (x >= 0 && (int64_t)x < V) ? label[x] : x; };
    auto sweep = [&](int which) {                                               // 0: every edge, 1: inside a tile, 2: between tiles
        bool any = false;
        for (int64_t v = 0; v < V; v++) {
            if (label[v] < 0) continue;
            int64_t i[3];
            pc_coords(v, n, i);
            for (int k = PC_NO_OFFSET + 1; k < 27; k++) {
                if (!pc_offset_in(conn, k)) continue;
                int code;
                const int64_t u = pc_edge(i, n, k, &code);
                if (!pc_is_interior_forward(k, code) || label[u] < 0) continue;
                if (which) {
                    int64_t j[3];
                    pc_coords(u, n, j);
                    const bool same = pc_tile_of(i, tiles) == pc_tile_of(j, tiles);
                    if (same != (which == 1)) continue;
                }
                int nd, value;
                if (pg_hook(label[v], label[u], &nd, &value)) {
                    any = true;
                    if (value < label[nd]) label[nd] = value;
                }
            }
        }
        for (int64_t v = 0; v < V; v++)
            if (label[v] >= 0) label[v] = pg_compress(get, (int)v);
        return any;
    };
    int64_t rounds = 1;
    if (tile_first) {
        while (sweep(1)) {}
        while (sweep(2)) rounds++;
        rounds++;                                                               // and the fixed point is taken from a round over every edge
    }
    while (sweep(0)) rounds++;
    return rounds;
}

// every seam edge with both ends in the set, once
inline void pc_seam_serial(const int64_t *n, int conn, const int32_t *label, std::vector<int32_t> &rec)
{
    const int64_t V = n[0] * n[1] * n[2];
    for (int64_t v = 0; v < V; v++) {
        if (label[v] < 0) continue;
        int64_t i[3];
        pc_coords(v, n, i);
        for (int k = 0; k < 27; k++) {
            if (k == PC_NO_OFFSET || !pc_offset_in(conn, k)) continue;
            int code;
            const int64_t u = pc_edge(i, n, k, &code);
            if (!pc_is_seam_forward(code) || label[u] < 0) continue;
            rec.push_back(label[v]); rec.push_back(label[u]); rec.push_back(code);
        }
    }
}

// the pairs of the quotient on the open labels: every voxel takes the label of its label
inline void pc_relabel_serial(int64_t V, const std::vector<int32_t> &pairs, int32_t *label)
{
    for (size_t p = 0; p + 1 < pairs.size(); p += 2) label[pairs[p]] = pairs[p + 1];
    for (int64_t v = 0; v < V; v++)
        if (label[v] >= 0) label[v] = label[label[v]];
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------

struct PcPlan {
    int64_t V;
    int64_t tiles[3], n_tiles;
    int64_t lds_bytes;                            // of the tile kernel
    int64_t seam_max;                             // seam records of the full grid: no set has more
    int64_t form;                                 // PC_FORM_GLOBAL or PC_FORM_TILE
    int64_t blocks;                               // workgroups of a kernel with a thread per voxel
    int64_t workspace;                            // bytes of the buffer of sit_percolation_levels
    const char *err;
};

// (voxel, offset) pairs of the connectivity whose shift is lexicographically positive
inline int64_t pc_seam_max(const int64_t *n, int conn)
{
    int64_t total = 0;
    for (int k = 0; k < 27; k++) {
        if (k == PC_NO_OFFSET || !pc_offset_in(conn, k)) continue;
        int d[3];
        pc_offset(k, d);
        int64_t zero[3], plus[3], all[3];                                       // indices along an axis with shift 0, +1, any
        for (int a = 0; a < 3; a++) {
            all[a] = n[a];
            plus[a] = d[a] > 0 ? 1 : 0;                                         // i = n - 1
            zero[a] = d[a] == 0 ? n[a] : n[a] - 1;                              // d = -1: all but i = 0
        }
        total += plus[0] * all[1] * all[2] + zero[0] * (plus[1] * all[2] + zero[1] * plus[2]);
    }
    return total;
}

struct PcPieces {
    double *grid; int32_t *label; unsigned long long *words; int32_t *seam;
    int64_t head;                                 // what sit_percolation_components takes beside begins here
    int32_t *size; unsigned *block_count; unsigned long long *offsets; int64_t *out;
};

// cap < 0: the buffer of sit_percolation_levels, without the pieces of the component records
inline PcPieces pc_layout(Carve &cv, const PcPlan &p, int64_t cap)
{
    PcPieces w;
    w.grid = cv.take<double>(p.V, 256);
    w.label = cv.take<int32_t>(p.V, 256);
    w.words = cv.take<unsigned long long>(PC_WORDS, 256);
    w.seam = cv.take<int32_t>(3 * p.seam_max, 256);
    cv.take<char>(0, 256);
    w.head = cv.used;
    w.size = cv.take<int32_t>(cap < 0 ? 0 : p.V, 256);
    w.block_count = cv.take<unsigned>(cap < 0 ? 0 : p.blocks, 256);
    w.offsets = cv.take<unsigned long long>(cap < 0 ? 0 : p.blocks + 1, 256);
    w.out = cv.take<int64_t>(cap < 0 ? 0 : 2 * cap, 256);
    cv.take<char>(0, 256);
    return w;
}

inline PcPlan pc_plan(const int64_t *n, int conn, int form)
{
    PcPlan p = PcPlan();
    for (int a = 0; a < 3; a++)
        if (n[a] < 1 || n[a] > PC_MAX_GRID) { p.err = "an axis of the grid holds 1 to 1024 voxels"; return p; }
    p.V = n[0] * n[1] * n[2];
    if (p.V > PC_MAX_VOXELS) { p.err = "more than 2^27 voxels"; return p; }
    if (!pc_connectivity_ok(conn)) { p.err = "connectivity is 6, 18 or 26"; return p; }
    if (form < 0 || form > 2) { p.err = "form is 0, 1 or 2"; return p; }
    const int64_t tile[3] = {PC_TILE0, PC_TILE1, PC_TILE2};
    for (int a = 0; a < 3; a++) p.tiles[a] = (n[a] + tile[a] - 1) / tile[a];
    p.n_tiles = p.tiles[0] * p.tiles[1] * p.tiles[2];
    p.lds_bytes = PC_TILE_VOXELS * 4;
    p.seam_max = pc_seam_max(n, conn);
    // form 0: the tile-local phase - on the 160 x 176 x 192 grid the 37 passes of the level search took 90.6 ms
    // with it, its confirming rounds included, and 98.3 ms with plain global rounds, the calls of either spread by under 1 ms
    p.form = form ? form : PC_FORM_TILE;
    p.blocks = (p.V + PC_THREADS - 1) / PC_THREADS;
    Carve cv = {nullptr, 0};
    pc_layout(cv, p, -1);
    p.workspace = cv.used;
    return p;
}

// ---- the two calls, serially: what the tests pin and what the device is measured against -------------------------------------------

// the periodic labels of {g >= level} into label [V] and the quotient; false: pc_quotient's refusal
inline bool pc_components_serial(const double *grid, const int64_t *n, double level, int conn, bool tile_first, int32_t *label, PcQuotient &q,
                                 int64_t *rounds, int64_t *n_rec)
{
    const int64_t V = n[0] * n[1] * n[2];
    std::vector<int32_t> rec;
    pc_init_serial(grid, V, level, label);
    *rounds = pc_label_serial(n, conn, tile_first, label);
    pc_seam_serial(n, conn, label, rec);
    *n_rec = (int64_t)rec.size() / 3;
    if (!pc_quotient(rec.data(), *n_rec, false, q)) return false;
    pc_relabel_serial(V, q.pairs, label);
    return true;
}

// the smallest (above) and the largest (top) pattern of the positive values at or above lo_bits and the largest under it (below); 0: none
inline void pc_range_serial(const double *grid, int64_t V, uint64_t lo_bits, uint64_t *above, uint64_t *top, uint64_t *below)
{
    *above = ~(uint64_t)0; *top = 0; *below = 0;
    for (int64_t v = 0; v < V; v++) {
        if (!(grid[v] > 0.0)) continue;
        const uint64_t b = pc_bits(grid[v]);
        if (!pc_candidate(grid[v], lo_bits)) { if (b > *below) *below = b; continue; }
        if (b < *above) *above = b;
        if (b > *top) *top = b;
    }
    if (*top == 0) *above = 0;
}

inline bool pc_levels_serial(const double *grid, const int64_t *n, int conn, bool tile_first, double *levels3, int32_t *ranks3, int64_t *passes)
{
    const int64_t V = n[0] * n[1] * n[2];
    std::vector<int32_t> label((size_t)V), rec;
    uint64_t above, top, below;
    pc_range_serial(grid, V, 1, &above, &top, &below);
    PcSearch s;
    pc_search_init(s, above, top);
    PcQuotient q;
    *passes = 0;
    for (uint64_t bits; pc_search_next(s, &bits);) {
        (*passes)++;
        rec.clear();
        pc_init_serial(grid, V, pc_value(bits), label.data());
        pc_label_serial(n, conn, tile_first, label.data());
        pc_seam_serial(n, conn, label.data(), rec);
        if (!pc_quotient(rec.data(), (int64_t)rec.size() / 3, true, q)) return false;
        pc_range_serial(grid, V, bits, &above, &top, &below);
        pc_search_update(s, q.max_rank, above, below);
    }
    for (int d = 0; d < 3; d++) {                                               // known_true is a snap: the bytes of a voxel's value
        levels3[d] = s.known_true[d] ? pc_value(s.known_true[d]) : 0.0;
        ranks3[d] = s.known_true[d] ? s.rank_at[d] : 0;
    }
    return true;
}
