// DensityPercolation: the connected components of a superlevel set {g >= level} of a periodic grid, the rank and the Hermite normal
// form of every component's loop lattice, and the levels at which the set first connects across the cell in one, two and three
// dimensions.  Every decision - neighbours and shifts, which edges a pass looks at, the hook and compress rules, the quotient step,
// the bisection, the limits, the pieces of a call's buffer (pc_layout) - is in percolation_plan.h; this file has the launches.
//
//   k_pc_init      label[v] = v in the set, -1 outside (the global form)
//   k_pc_tile      the same for an 8 x 8 x 16 tile, whose interior edges are then brought to their fixed point in LDS (hook by an
//                  LDS atomic minimum, compress by pointer jumping, until a hook pass of the workgroup finds equal labels); the
//                  tile's voxels leave with the flat index of their local root (the tile form)
//   k_pc_hook      a thread per voxel, its interior edges towards the positive offsets - all of them, or those that leave the
//                  voxel's tile; k_pc_compress the pointer jumping.  The host reads one word per round; the tile form's last round
//                  looks at every edge again
//   k_pc_seam      the seam edges with both ends in the set as records (label_u, label_v, shift code), compacted by ballot
//   k_pc_relabel   the quotient's (open root, periodic root) pairs onto the roots; k_pc_flatten every voxel onto its root's label
//   k_pc_sizes     voxels per root (one integer add per wave and root); k_pc_roots / k_pc_scan / k_pc_compact the roots in
//                  ascending order with their sizes
//   k_pc_range     the smallest and the largest bit pattern of the positive values at or above a pattern and the largest under it:
//                  the range of the bisection and the two snaps of a probe
// Every kernel is a finite launch.  Labels that other workgroups of a launch lower are read and written with agent-scope atomics
// only (a stale value is a valid, merely older, label: the rules are monotonic).  Integer atomics only: the same bytes on every call.
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "sit_internal.h"
#include "percolation_plan.h"
#include "sitator_hip_percolation.h"

struct PcGrid { i64 n[3], V, tiles[3]; };

namespace {
__device__ __forceinline__ int pc_load(const i32 *label, i64 x)
{
    return __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int pc_load_lds(const i32 *lab, int x)
{
    return __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
}

__global__ __launch_bounds__(PC_THREADS) void k_pc_init(const double *grid, i64 V, double level, i32 *label)
{
    const i64 v = (i64)blockIdx.x * PC_THREADS + threadIdx.x;
    if (v < V) label[v] = pc_in_set(grid[v], level) ? (i32)v : -1;
}

// grid: the tiles
__global__ __launch_bounds__(PC_THREADS) void k_pc_tile(const double *grid, PcGrid g, double level, int conn, i32 *label)
{
    __shared__ i32 lab[PC_TILE_VOXELS];
    const i64 t = blockIdx.x, t2 = t % g.tiles[2], t1 = (t / g.tiles[2]) % g.tiles[1], t0 = t / (g.tiles[1] * g.tiles[2]);
    const i64 o0 = t0 * PC_TILE0, o1 = t1 * PC_TILE1, o2 = t2 * PC_TILE2;
    for (int k = 0; k < PC_PER_THREAD; k++) {
        const int x = threadIdx.x + k * PC_THREADS;
        const i64 i0 = o0 + x / (PC_TILE1 * PC_TILE2), i1 = o1 + x / PC_TILE2 % PC_TILE1, i2 = o2 + x % PC_TILE2;
        const bool live = i0 < g.n[0] && i1 < g.n[1] && i2 < g.n[2];
        lab[x] = live && pc_in_set(grid[(i0 * g.n[1] + i1) * g.n[2] + i2], level) ? x : -1;
    }
    __syncthreads();
    while (true) {                                               // every round with a hook lowers a label: finite
        int hooked = 0;
        for (int k = 0; k < PC_PER_THREAD; k++) {
            const int x = threadIdx.x + k * PC_THREADS;
            const int lu = pc_load_lds(lab, x);
            if (lu < 0) continue;
            const int l0 = x / (PC_TILE1 * PC_TILE2), l1 = x / PC_TILE2 % PC_TILE1, l2 = x % PC_TILE2;
            for (int f = PC_NO_OFFSET + 1; f < 27; f++) {
                if (!pc_offset_in(conn, f)) continue;
                int d[3];
                pc_offset(f, d);
                const int m0 = l0 + d[0], m1 = l1 + d[1], m2 = l2 + d[2];
                if (m0 < 0 || m0 >= PC_TILE0 || m1 < 0 || m1 >= PC_TILE1 || m2 < 0 || m2 >= PC_TILE2) continue;      // leaves the tile
                if (o0 + m0 >= g.n[0] || o1 + m1 >= g.n[1] || o2 + m2 >= g.n[2]) continue;                          // leaves the grid: a seam edge
                const int lv = pc_load_lds(lab, (m0 * PC_TILE1 + m1) * PC_TILE2 + m2);
                int node, value;
                if (lv < 0 || !pg_hook(lu, lv, &node, &value)) continue;
                hooked = 1;
                if (node >= 0 && node < PC_TILE_VOXELS) __hip_atomic_fetch_min(lab + node, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        for (int k = 0; k < PC_PER_THREAD; k++) {
            const int x = threadIdx.x + k * PC_THREADS;
            const int own = pc_load_lds(lab, x);
            if (own < 0) continue;
            const int p = pg_compress([&](int y) { return (y >= 0 && y < PC_TILE_VOXELS) ? pc_load_lds(lab, y) : y; }, x);
            if (p != own) __hip_atomic_store(lab + x, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (!__syncthreads_or(hooked)) break;
    }
    for (int k = 0; k < PC_PER_THREAD; k++) {
        const int x = threadIdx.x + k * PC_THREADS;
        const i64 i0 = o0 + x / (PC_TILE1 * PC_TILE2), i1 = o1 + x / PC_TILE2 % PC_TILE1, i2 = o2 + x % PC_TILE2;
        if (!(i0 < g.n[0] && i1 < g.n[1] && i2 < g.n[2])) continue;
        const int r = lab[x];
        i32 out = -1;
        if (r >= 0 && r < PC_TILE_VOXELS)                         // the local order is the order of the flat indices: the lowest stays the lowest
            out = (i32)(((o0 + r / (PC_TILE1 * PC_TILE2)) * g.n[1] + o1 + r / PC_TILE2 % PC_TILE1) * g.n[2] + o2 + r % PC_TILE2);
        label[(i0 * g.n[1] + i1) * g.n[2] + i2] = out;
    }
}

// cross_only: the edges inside a tile are at their fixed point already
__global__ __launch_bounds__(PC_THREADS) void k_pc_hook(i32 *label, PcGrid g, int conn, int cross_only, unsigned *changed)
{
    const i64 v = (i64)blockIdx.x * PC_THREADS + threadIdx.x;
    bool hooked = false;
    const int lu = v < g.V ? pc_load(label, v) : -1;
    if (lu >= 0) {
        i64 i[3];
        pc_coords(v, g.n, i);
        for (int f = PC_NO_OFFSET + 1; f < 27; f++) {
            if (!pc_offset_in(conn, f)) continue;
            int code;
            const i64 u = pc_edge(i, g.n, f, &code);
            if (!pc_is_interior_forward(f, code)) continue;
            if (cross_only) {
                i64 j[3];
                pc_coords(u, g.n, j);
                if (pc_tile_of(i, g.tiles) == pc_tile_of(j, g.tiles)) continue;
            }
            const int lv = pc_load(label, u);
            int node, value;
            if (lv < 0 || !pg_hook(lu, lv, &node, &value)) continue;
            hooked = true;
            // a label is a voxel of the grid; it is checked all the same before it is used as an index
            if (node >= 0 && (i64)node < g.V) __hip_atomic_fetch_min(label + node, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const unsigned long long m = __ballot(hooked);
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) __hip_atomic_store(changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(PC_THREADS) void k_pc_compress(i32 *label, i64 V)
{
    const i64 v = (i64)blockIdx.x * PC_THREADS + threadIdx.x;
    if (v >= V) return;
    const int own = pc_load(label, v);
    if (own < 0) return;
    const int p = pg_compress([&](int x) { return (x >= 0 && (i64)x < V) ? pc_load(label, x) : x; }, (int)v);
    if (p != own) __hip_atomic_store(label + v, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// rec [cap][3]; *cursor counts every record, also those beyond cap (the plan's cap holds them all)
__global__ __launch_bounds__(PC_THREADS) void k_pc_seam(const i32 *label, PcGrid g, int conn, i32 *rec, unsigned cap, unsigned *cursor)
{
    const i64 v = (i64)blockIdx.x * PC_THREADS + threadIdx.x;
    const int lu = v < g.V ? label[v] : -1;
    i64 i[3] = {0, 0, 0};
    bool face = false;
    if (lu >= 0) {
        pc_coords(v, g.n, i);
        face = i[0] == g.n[0] - 1 || i[1] == g.n[1] - 1 || i[2] == g.n[2] - 1;      // a positive shift needs the upper end of an axis
    }
    if (!__ballot(face)) return;
    const int lane = threadIdx.x & 63;
    for (int f = 0; f < 27; f++) {
        if (f == PC_NO_OFFSET || !pc_offset_in(conn, f)) continue;
        int code = PC_NO_OFFSET, lv = -1;
        if (face) {
            const i64 u = pc_edge(i, g.n, f, &code);
            if (pc_is_seam_forward(code)) lv = label[u];
        }
        const bool on = lv >= 0;
        const unsigned long long m = __ballot(on);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(cursor, (unsigned)__popcll(m));
        base = __shfl(base, leader);
        if (on) {
            const unsigned at = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            if (at < cap) { rec[3 * (i64)at] = lu; rec[3 * (i64)at + 1] = lv; rec[3 * (i64)at + 2] = code; }
        }
    }
}

__global__ __launch_bounds__(PC_THREADS) void k_pc_relabel(const i32 *pairs, i64 n_pairs, i64 V, i32 *label)
{
    const i64 p = (i64)blockIdx.x * PC_THREADS + threadIdx.x;
    if (p >= n_pairs) return;
    const i32 from = pairs[2 * p], to = pairs[2 * p + 1];
    if (from >= 0 && (i64)from < V && to >= 0 && to < from) label[from] = to;
}

// after k_pc_relabel a chain has two steps at most: voxel -> open root -> periodic root
__global__ __launch_bounds__(PC_THREADS) void k_pc_flatten(i32 *label, i64 V)
{
    const i64 v = (i64)blockIdx.x * PC_THREADS + threadIdx.x;
    if (v >= V) return;
    const int own = pc_load(label, v);
    if (own < 0 || (i64)own >= V) return;
    const int top = pc_load(label, own);
    if (top >= 0 && top != own) __hip_atomic_store(label + v, top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// size[root] = voxels with that label: the lanes of a wave that share the first live lane's root add once
__global__ __launch_bounds__(PC_THREADS) void k_pc_sizes(const i32 *label, i64 V, i32 *size)
{
    const i64 v = (i64)blockIdx.x * PC_THREADS + threadIdx.x;
    int root = v < V ? label[v] : -1;
    if (root >= 0 && (i64)root >= V) root = -1;
    const int lane = threadIdx.x & 63;
    unsigned long long left = __ballot(root >= 0);
    while (left) {
        const int leader = __ffsll((long long)left) - 1;
        const int r = __shfl(root, leader);
        const unsigned long long same = __ballot(root == r) & left;
        if (lane == leader) atomicAdd(size + r, (i32)__popcll(same));
        left &= ~same;
    }
}

__global__ __launch_bounds__(PC_THREADS) void k_pc_roots(const i32 *label, i64 V, unsigned *block_count)
{
    const i64 v = (i64)blockIdx.x * PC_THREADS + threadIdx.x;
    const int n = __syncthreads_count(v < V && (i64)label[v] == v);
    if (threadIdx.x == 0) block_count[blockIdx.x] = (unsigned)n;
}

// one workgroup: offsets[b] = roots of the workgroups before b; offsets[nb] = all
__global__ __launch_bounds__(PC_THREADS) void k_pc_scan(const unsigned *block_count, i64 nb, u64 *offsets)
{
    __shared__ u64 part[PC_THREADS];
    const i64 chunk = (nb + PC_THREADS - 1) / PC_THREADS, lo = (i64)threadIdx.x * chunk, hi = lo + chunk < nb ? lo + chunk : nb;
    u64 sum = 0;
    for (i64 b = lo; b < hi; b++) sum += block_count[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    u64 before = 0;
    for (int j = 0; j < (int)threadIdx.x; j++) before += part[j];
    for (i64 b = lo; b < hi; b++) { offsets[b] = before; before += block_count[b]; }
    if (threadIdx.x == PC_THREADS - 1) offsets[nb] = before;      // lo >= nb for the threads beyond the last chunk: `before` is the total
}

// out [cap][2]: (root, size) in ascending root
__global__ __launch_bounds__(PC_THREADS) void k_pc_compact(const i32 *label, const i32 *size, const u64 *offsets, i64 V, i64 cap, i64 *out)
{
    __shared__ unsigned wave_n[PC_THREADS / 64];
    const i64 v = (i64)blockIdx.x * PC_THREADS + threadIdx.x;
    const bool on = v < V && (i64)label[v] == v;
    const unsigned long long m = __ballot(on);
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    if (lane == 0) wave_n[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (!on) return;
    u64 rank = offsets[blockIdx.x] + (u64)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) rank += wave_n[w];
    if ((i64)rank < cap) { out[2 * rank] = v; out[2 * rank + 1] = (i64)size[v]; }
}

// words = {min, max of the bit patterns of the positive values at or above lo_bits (pc_candidate), max of those under it}; the caller
// sets ~0, 0, 0
__global__ __launch_bounds__(PC_THREADS) void k_pc_range(const double *grid, i64 V, u64 lo_bits, u64 *words)
{
    u64 lo = ~0ull, hi = 0, under = 0;
    for (i64 v = (i64)blockIdx.x * PC_THREADS + threadIdx.x; v < V; v += (i64)gridDim.x * PC_THREADS) {
        const double x = grid[v];
        if (!(x > 0.0)) continue;
        const u64 b = pc_bits(x);
        if (!pc_candidate(x, lo_bits)) { under = b > under ? b : under; continue; }
        lo = b < lo ? b : lo;
        hi = b > hi ? b : hi;
    }
    for (int s = 32; s > 0; s >>= 1) {
        const u64 a = (u64)__shfl_xor((long long)lo, s), b = (u64)__shfl_xor((long long)hi, s), c = (u64)__shfl_xor((long long)under, s);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
        under = c > under ? c : under;
    }
    if ((threadIdx.x & 63) == 0) {
        if (hi) { atomicMin(words, lo); atomicMax(words + 1, hi); }
        if (under) atomicMax(words + 2, under);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------

static inline unsigned pc_blocks(i64 n) { return (unsigned)((n + PC_THREADS - 1) / PC_THREADS); }

extern "C" int sit_percolation_plan(const i64 *grid3, int connectivity, int form, i64 *out12)
{
    if (!grid3 || !out12) return SIT_ERR_INVALID;
    const PcPlan p = pc_plan(grid3, connectivity, form);
    const i64 out[12] = {PC_THREADS, PC_TILE0, PC_TILE1, PC_TILE2, p.lds_bytes, p.n_tiles, p.form, p.seam_max, p.workspace, p.V, p.blocks,
                         PC_RECORD_WORDS};
    for (int i = 0; i < 12; i++) out12[i] = out[i];
    return p.err ? SIT_ERR_INVALID : SIT_OK;
}

struct PcCall {
    PcPlan plan;
    PcGrid g;
    PcPieces w;
    int conn;
    std::vector<i32> rec;                                        // the seam records of the last pass
    i64 rounds, n_rec;
};

static int pc_begin(sit_ctx *c, const char *who, const double *grid, const i64 *grid3, int conn, int form, i64 cap, Scoped *work, PcCall *call)
{
    call->plan = pc_plan(grid3, conn, form);
    if (call->plan.err) { c->msg = std::string(who) + ": " + call->plan.err; return SIT_ERR_INVALID; }
    for (int a = 0; a < 3; a++) { call->g.n[a] = grid3[a]; call->g.tiles[a] = call->plan.tiles[a]; }
    call->g.V = call->plan.V;
    call->conn = conn;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = carve_scratch(c, [&](Carve &cv) { call->w = pc_layout(cv, call->plan, cap); }, work))) return rc;
    return copy_to_device(c, call->w.grid, grid, (size_t)call->plan.V * 8);
}

// the open-boundary labels of {g >= level} and the seam records between them, on the host
static int pc_pass(sit_ctx *c, PcCall *k, double level)
{
    const PcPlan &p = k->plan;
    unsigned *words = (unsigned *)k->w.words;                    // [0]: the change flag, [2]: the seam cursor
    unsigned *h_words = (unsigned *)c->h_pinned;
    if (p.form == PC_FORM_TILE) k_pc_tile<<<dim3((unsigned)p.n_tiles), dim3(PC_THREADS), 0, c->stream>>>(k->w.grid, k->g, level, k->conn, k->w.label);
    else k_pc_init<<<dim3(pc_blocks(p.V)), dim3(PC_THREADS), 0, c->stream>>>(k->w.grid, p.V, level, k->w.label);
    HIP_TRY(c, hipGetLastError());
    k->rounds = 0;
    bool settled = false;
    // the tile form's rounds look at the edges between tiles only, which rests on every voxel of a tile's component leaving a compress
    // with one label - true unless a chain outgrew PG_JUMP_CAP while others shortened it.  So the round that finds those edges at rest
    // is followed by one over every edge, and the fixed point is accepted from a round that looked at all of them
    int cross_only = p.form == PC_FORM_TILE ? 1 : 0;
    while (k->rounds < p.V + 2) {                                // a component of n voxels is joined after fewer rounds than that
        k->rounds++;
        HIP_TRY(c, hipMemsetAsync(words, 0, 16, c->stream));
        k_pc_hook<<<dim3(pc_blocks(p.V)), dim3(PC_THREADS), 0, c->stream>>>(k->w.label, k->g, k->conn, cross_only, words);
        k_pc_compress<<<dim3(pc_blocks(p.V)), dim3(PC_THREADS), 0, c->stream>>>(k->w.label, p.V);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h_words, words, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (h_words[0]) continue;
        if (!cross_only) { settled = true; break; }
        cross_only = 0;
    }
    if (!settled) { c->msg = "sit_percolation: the labelling did not settle within as many rounds as the grid has voxels"; return SIT_ERR_CAPACITY; }
    k_pc_seam<<<dim3(pc_blocks(p.V)), dim3(PC_THREADS), 0, c->stream>>>(k->w.label, k->g, k->conn, k->w.seam, (unsigned)p.seam_max, words + 2);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(h_words, words + 2, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    k->n_rec = (i64)h_words[0];
    if (k->n_rec > p.seam_max) { c->msg = "sit_percolation: more seam records than the grid has seam edges"; return SIT_ERR_CAPACITY; }
    k->rec.resize((size_t)(3 * k->n_rec));
    if (k->n_rec > 0) {
        HIP_TRY(c, hipMemcpyAsync(k->rec.data(), k->w.seam, (size_t)k->n_rec * 12, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return SIT_OK;
}

extern "C" int sit_percolation_components(sit_ctx *c, const double *grid, const i64 *grid3, double level, int connectivity, int form,
                                          int32_t *labels, i64 cap, i64 *records, i64 *n_out, i64 *info4)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, grid && grid3 && n_out && info4 && cap >= 0 && (records || cap == 0), "sit_percolation_components: missing array or a negative cap");
    SIT_REQUIRE(c, level == level, "sit_percolation_components: the level is not a number");
    const PcPlan sized = pc_plan(grid3, connectivity, form);
    if (!sized.err && cap > sized.V) cap = sized.V;
    Scoped work(c);
    PcCall k;
    int rc;
    if ((rc = pc_begin(c, "sit_percolation_components", grid, grid3, connectivity, form, cap, &work, &k))) return rc;
    if ((rc = pc_pass(c, &k, level))) return rc;
    PcQuotient q;
    if (!pc_quotient(k.rec.data(), k.n_rec, false, q)) { c->msg = "sit_percolation_components: a loop lattice beyond int32"; return SIT_ERR_CAPACITY; }
    const i64 V = k.plan.V, nb = k.plan.blocks, n_pairs = (i64)q.pairs.size() / 2;
    Scoped pairs(c);
    if (n_pairs > 0) {
        HIP_TRY(c, sit_dmalloc(c, &pairs.p, (size_t)n_pairs * 8));
        if ((rc = copy_to_device(c, pairs.p, q.pairs.data(), (size_t)n_pairs * 8))) return rc;
        k_pc_relabel<<<dim3(pc_blocks(n_pairs)), dim3(PC_THREADS), 0, c->stream>>>((const i32 *)pairs.p, n_pairs, V, k.w.label);
        k_pc_flatten<<<dim3(pc_blocks(V)), dim3(PC_THREADS), 0, c->stream>>>(k.w.label, V);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemsetAsync(k.w.size, 0, (size_t)V * 4, c->stream));
    k_pc_sizes<<<dim3(pc_blocks(V)), dim3(PC_THREADS), 0, c->stream>>>(k.w.label, V, k.w.size);
    k_pc_roots<<<dim3((unsigned)nb), dim3(PC_THREADS), 0, c->stream>>>(k.w.label, V, k.w.block_count);
    k_pc_scan<<<dim3(1), dim3(PC_THREADS), 0, c->stream>>>(k.w.block_count, nb, (u64 *)k.w.offsets);
    k_pc_compact<<<dim3((unsigned)nb), dim3(PC_THREADS), 0, c->stream>>>(k.w.label, k.w.size, (const u64 *)k.w.offsets, V, cap, k.w.out);
    HIP_TRY(c, hipGetLastError());
    u64 *h_total = (u64 *)c->h_pinned;
    HIP_TRY(c, hipMemcpyAsync(h_total, k.w.offsets + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const i64 n = (i64)h_total[0], fetch = n < cap ? n : cap;
    *n_out = n;
    if (fetch > 0) {
        std::vector<i64> pairs_out((size_t)(2 * fetch));
        HIP_TRY(c, hipMemcpyAsync(pairs_out.data(), k.w.out, (size_t)fetch * 16, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::unordered_map<i32, size_t> with_loops;
        for (size_t j = 0; j < q.comps.size(); j++) with_loops.emplace(q.comps[j].root, j);
        for (i64 j = 0; j < fetch; j++) {
            i64 *r = records + PC_RECORD_WORDS * j;
            for (int x = 0; x < PC_RECORD_WORDS; x++) r[x] = 0;
            r[0] = pairs_out[(size_t)(2 * j)]; r[1] = pairs_out[(size_t)(2 * j + 1)];
            const auto it = with_loops.find((i32)r[0]);
            if (it == with_loops.end()) continue;
            r[2] = q.comps[it->second].rank;
            for (int x = 0; x < 9; x++) r[3 + x] = q.comps[it->second].basis[x];
        }
    }
    if (labels && (rc = copy_to_host(c, labels, k.w.label, (size_t)V * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // the buffers go back to the pool
    info4[0] = k.rounds; info4[1] = k.n_rec; info4[2] = k.plan.form; info4[3] = q.distinct;
    return SIT_OK;
}

// words + 4: the three patterns of k_pc_range, on the host (0: none)
static int pc_range(sit_ctx *c, PcCall *k, uint64_t lo_bits, uint64_t *above, uint64_t *top, uint64_t *below)
{
    u64 *words = (u64 *)k->w.words + 4, *h = (u64 *)c->h_pinned;
    HIP_TRY(c, hipMemsetAsync(words, 0xFF, 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(words + 1, 0, 16, c->stream));
    const i64 want = (k->plan.V + 8 * PC_THREADS - 1) / (8 * PC_THREADS);
    k_pc_range<<<dim3((unsigned)(want < 1 ? 1 : want)), dim3(PC_THREADS), 0, c->stream>>>(k->w.grid, k->plan.V, lo_bits, words);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(h, words, 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *above = h[1] ? h[0] : 0; *top = h[1]; *below = h[2];
    return SIT_OK;
}

extern "C" int sit_percolation_levels(sit_ctx *c, const double *grid, const i64 *grid3, int connectivity, int form, double *levels3,
                                      int32_t *ranks3, i64 *info4)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, grid && grid3 && levels3 && ranks3 && info4, "sit_percolation_levels: missing array");
    Scoped work(c);
    PcCall k;
    int rc;
    if ((rc = pc_begin(c, "sit_percolation_levels", grid, grid3, connectivity, form, -1, &work, &k))) return rc;
    uint64_t above, top, below;
    if ((rc = pc_range(c, &k, 1, &above, &top, &below))) return rc;
    PcSearch s;
    pc_search_init(s, above, top);
    i64 passes = 0;
    k.rounds = 0; k.n_rec = 0;
    PcQuotient q;
    for (uint64_t bits; pc_search_next(s, &bits);) {
        passes++;
        if ((rc = pc_pass(c, &k, pc_value(bits)))) return rc;
        if (!pc_quotient(k.rec.data(), k.n_rec, true, q)) { c->msg = "sit_percolation_levels: a loop lattice beyond int32"; return SIT_ERR_CAPACITY; }
        if ((rc = pc_range(c, &k, bits, &above, &top, &below))) return rc;        // the snaps: min{g[v] : g[v] >= level} and max{g[v] : g[v] < level}
        pc_search_update(s, q.max_rank, above, below);
    }
    for (int d = 0; d < 3; d++) {                                // known_true is a snap: the bytes of a voxel's value
        levels3[d] = s.known_true[d] ? pc_value(s.known_true[d]) : 0.0;
        ranks3[d] = s.known_true[d] ? s.rank_at[d] : 0;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    info4[0] = passes; info4[1] = k.rounds; info4[2] = k.n_rec; info4[3] = k.plan.form;
    return SIT_OK;
}
