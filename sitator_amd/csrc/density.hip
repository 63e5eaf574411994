// IonicDensity: the time-averaged probability density of chosen atoms on a periodic grid, as integer counts per voxel (and per
// class of the site an ion is assigned to), from the frames as they lie in device memory; a smoothing of the counts by a list
// of taps; the peaks of a grid.  Every decision - the voxel of a point, the plane of a label, the slot of a key, the peak rule,
// the limits, the runs and windows a workspace cap allows, the pieces of a call's buffer (dn_layout) - is in density_plan.h.
//
//   k_dn_count     a workgroup takes a run of DN_RUN taken frames of the selection.  Entries are aggregated in an LDS
//                  open-addressing table keyed by plane x V + voxel (key by compare-and-swap, count by add; a thread first
//                  folds consecutive entries of one key in a register); an entry that finds no slot within DN_PROBE goes to
//                  memory on its own; every occupied slot is flushed with one 64-bit add.  table == 0: the same kernel, one
//                  64-bit add in memory per entry
//   k_dn_smooth    a 4 x 8 x 8 tile of voxels of a plane: the counts of the tile and its halo are staged in LDS as doubles, a
//                  thread walks the taps in list order; a tile whose staged counts are all zero writes +0
//   k_dn_peaks     the peak rule per voxel, a flag and a count per workgroup; k_dn_scan the offsets; k_dn_compact the indices
// Integer atomics only: the same bytes on every call and in every form.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "series.h"
#include "density_plan.h"
#include "sitator_hip_density.h"

extern __shared__ __align__(16) double dn_tile[];      // k_dn_smooth: DnPlan::smooth_lds bytes

struct DnGrid { i64 n[3], V; };

struct DnLabels {
    const i64 *labels;             // [F][M] the resident labels, or null: one plane
    i64 M, K;
    const i32 *site_class;         // [K]
    i64 n_classes;
};

struct DnRun {
    i64 j0, nj;                    // the taken frames of this launch: [j0, j0 + nj)
    i64 stride;
    i64 f0;                        // the frame the source's first one is
};

// n entries of a key into the table, or - no slot within the probe limit, or no table - into memory
__device__ __forceinline__ void dn_add(uint32_t *keys, uint32_t *cnt, int table, uint32_t key, uint32_t n, u64 *counts)
{
    if (table) {
        const uint32_t slot = dn_slot(key);
        for (int i = 0; i < DN_PROBE; i++) {
            const uint32_t s = dn_probe(slot, i);
            const uint32_t seen = atomicCAS(&keys[s], DN_EMPTY, key);
            if (seen == DN_EMPTY || seen == key) { atomicAdd(&cnt[s], n); return; }
        }
    }
    atomicAdd(counts + key, (u64)n);
}

// grid: runs of DN_RUN taken frames of the launch.  status: {largest label beyond the sites + 1, labels below -1, skipped}
__global__ __launch_bounds__(DN_THREADS) void k_dn_count(SeriesSource src, i64 n_sel, DnRun r, MsdCell cell, DnGrid g, DnLabels lb, int table,
                                                         u64 *counts, u64 *status)
{
    __shared__ uint32_t keys[DN_SLOTS], cnt[DN_SLOTS];
    __shared__ u64 s_status[3];
    const i64 jb = (i64)blockIdx.x * DN_RUN;
    if (jb >= r.nj) return;
    const i64 nfr = r.nj - jb < DN_RUN ? r.nj - jb : DN_RUN, entries = nfr * n_sel;
    for (int s = threadIdx.x; s < DN_SLOTS; s += DN_THREADS) { keys[s] = DN_EMPTY; cnt[s] = 0; }
    if (threadIdx.x < 3) s_status[threadIdx.x] = 0;
    __syncthreads();
    // few atoms: a thread follows one atom through consecutive frames (an ion rattles in its voxel: one table add per stay);
    // many: the atoms of a frame across the lanes
    const bool chunked = n_sel < DN_THREADS;
    const i64 chunk = (entries + DN_THREADS - 1) / DN_THREADS;
    u64 skipped = 0, beyond = 0, below = 0;
    uint32_t run_key = DN_EMPTY, run_n = 0;
    for (i64 k = 0; k < chunk; k++) {
        const i64 e = chunked ? (i64)threadIdx.x * chunk + k : (i64)threadIdx.x + k * DN_THREADS;
        if (e >= entries) break;
        const i64 i = chunked ? e / nfr : e % n_sel, f = chunked ? e - i * nfr : e / n_sel;
        const i64 frame = (r.j0 + jb + f) * r.stride;
        i64 plane = 0;
        if (lb.labels) {
            const i64 l = lb.labels[frame * lb.M + i];
            if (l >= lb.K) { if ((u64)l + 1 > beyond) beyond = (u64)l + 1; continue; }
            if (l < -1) { below++; continue; }
            plane = dn_plane(l, lb.site_class, lb.n_classes);
        }
        const double *p = src.at(frame - r.f0, i);
        const i64 v = dn_voxel(cell.ci, g.n, p[0], p[1], p[2]);
        if (v < 0) { skipped++; continue; }
        const uint32_t key = (uint32_t)(plane * g.V + v);
        if (!table) { atomicAdd(counts + key, 1ull); continue; }
        if (key == run_key) { run_n++; continue; }
        if (run_n) dn_add(keys, cnt, table, run_key, run_n, counts);
        run_key = key; run_n = 1;
    }
    if (run_n) dn_add(keys, cnt, table, run_key, run_n, counts);
    if (beyond) atomicMax(&s_status[0], beyond);
    if (below) atomicAdd(&s_status[1], below);
    if (skipped) atomicAdd(&s_status[2], skipped);
    __syncthreads();
    if (table)
        for (int s = threadIdx.x; s < DN_SLOTS; s += DN_THREADS)
            if (keys[s] != DN_EMPTY) atomicAdd(counts + keys[s], (u64)cnt[s]);
    if (threadIdx.x == 0) {
        if (s_status[0]) atomicMax(status, s_status[0]);
        if (s_status[1]) atomicAdd(status + 1, s_status[1]);
        if (s_status[2]) atomicAdd(status + 2, s_status[2]);
    }
}

struct DnSmooth {
    i64 n[3], V;
    i64 tiles[3];
    int ext[3], halo[3];
    int n_taps, lds;
};

// grid: (tiles of a plane, planes)
__global__ __launch_bounds__(DN_THREADS) void k_dn_smooth(const u64 *counts, const i32 *taps, const double *weights, DnSmooth s, double *out)
{
    const i64 t = blockIdx.x, t2 = t % s.tiles[2], t1 = (t / s.tiles[2]) % s.tiles[1], t0 = t / (s.tiles[1] * s.tiles[2]);
    const i64 o0 = t0 * DN_TILE0, o1 = t1 * DN_TILE1, o2 = t2 * DN_TILE2;
    const int l2 = threadIdx.x % DN_TILE2, l1 = (threadIdx.x / DN_TILE2) % DN_TILE1, l0 = threadIdx.x / (DN_TILE2 * DN_TILE1);
    const i64 i0 = o0 + l0, i1 = o1 + l1, i2 = o2 + l2;
    const bool live = i0 < s.n[0] && i1 < s.n[1] && i2 < s.n[2];
    const u64 *src = counts + (i64)blockIdx.y * s.V;
    double acc = 0.0;
    if (s.lds) {
        const int e1 = s.ext[1], e2 = s.ext[2], cells = s.ext[0] * e1 * e2;
        int any = 0;
        for (int c = threadIdx.x; c < cells; c += DN_THREADS) {
            const int a2 = c % e2, a1 = (c / e2) % e1, a0 = c / (e1 * e2);
            const i64 x0 = dn_wrap(o0 - s.halo[0] + a0, s.n[0]), x1 = dn_wrap(o1 - s.halo[1] + a1, s.n[1]);
            const i64 x2 = dn_wrap(o2 - s.halo[2] + a2, s.n[2]);
            const u64 v = src[(x0 * s.n[1] + x1) * s.n[2] + x2];
            any |= v != 0;
            dn_tile[c] = (double)v;
        }
        if (!__syncthreads_or(any)) {                             // every product is a zero: the sum from +0 is +0
            if (live) out[(i64)blockIdx.y * s.V + (i0 * s.n[1] + i1) * s.n[2] + i2] = 0.0;
            return;
        }
        const int base = ((l0 + s.halo[0]) * e1 + (l1 + s.halo[1])) * e2 + l2 + s.halo[2];
        for (int k = 0; k < s.n_taps; k++) {
            const int off = (taps[3 * k] * e1 + taps[3 * k + 1]) * e2 + taps[3 * k + 2];
            acc = acc + weights[k] * dn_tile[base + off];
        }
    } else if (live) {
        for (int k = 0; k < s.n_taps; k++) {
            const i64 x0 = dn_wrap(i0 + taps[3 * k], s.n[0]), x1 = dn_wrap(i1 + taps[3 * k + 1], s.n[1]);
            const i64 x2 = dn_wrap(i2 + taps[3 * k + 2], s.n[2]);
            acc = acc + weights[k] * (double)src[(x0 * s.n[1] + x1) * s.n[2] + x2];
        }
    }
    if (live) out[(i64)blockIdx.y * s.V + (i0 * s.n[1] + i1) * s.n[2] + i2] = acc;
}

__global__ __launch_bounds__(DN_THREADS) void k_dn_peaks(const double *grid, DnGrid g, double threshold, unsigned char *flag, unsigned *block_count)
{
    const i64 v = (i64)blockIdx.x * DN_THREADS + threadIdx.x;
    const int pk = v < g.V && dn_is_peak(grid, g.n, v, threshold) ? 1 : 0;
    if (v < g.V) flag[v] = (unsigned char)pk;
    const int n = __syncthreads_count(pk);
    if (threadIdx.x == 0) block_count[blockIdx.x] = (unsigned)n;
}

// one workgroup: offsets[b] = peaks of the workgroups before b; offsets[nb] = all
__global__ __launch_bounds__(DN_THREADS) void k_dn_scan(const unsigned *block_count, i64 nb, u64 *offsets)
{
    __shared__ u64 part[DN_THREADS];
    const i64 chunk = (nb + DN_THREADS - 1) / DN_THREADS, lo = (i64)threadIdx.x * chunk, hi = lo + chunk < nb ? lo + chunk : nb;
    u64 sum = 0;
    for (i64 b = lo; b < hi; b++) sum += block_count[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    u64 before = 0;
    for (int j = 0; j < (int)threadIdx.x; j++) before += part[j];
    for (i64 b = lo; b < hi; b++) { offsets[b] = before; before += block_count[b]; }
    if (threadIdx.x == DN_THREADS - 1) offsets[nb] = before;      // lo >= nb for the threads beyond the last chunk: `before` is the total
}

__global__ __launch_bounds__(DN_THREADS) void k_dn_compact(const unsigned char *flag, const u64 *offsets, i64 V, i64 cap, i64 *out)
{
    __shared__ unsigned wave_n[DN_THREADS / 64];
    const i64 v = (i64)blockIdx.x * DN_THREADS + threadIdx.x;
    const bool pk = v < V && flag[v];
    const unsigned long long m = __ballot(pk);
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    if (lane == 0) wave_n[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (!pk) return;
    u64 rank = offsets[blockIdx.x] + (u64)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) rank += wave_n[w];
    if ((i64)rank < cap) out[rank] = v;
}

// ---- host side ------------------------------------------------------------------------------------------------------------

static DnPlanIn dn_plan_in(i64 F, i64 A, i64 n_sel, i64 stride, const i64 *grid3, i64 K, i64 n_classes, i64 n_taps, const i64 *halo, i64 form,
                           bool host, i64 workspace_bytes)
{
    DnPlanIn in;
    in.F = F; in.A = A; in.n_sel = n_sel; in.stride = stride; in.K = K; in.n_classes = n_classes; in.n_taps = n_taps; in.form = form;
    for (int a = 0; a < 3; a++) { in.n[a] = grid3[a]; in.halo[a] = halo[a]; }
    in.host = host; in.workspace_bytes = workspace_bytes;
    return in;
}

extern "C" int sit_density_plan(i64 F, i64 A, i64 n_sel, i64 frame_stride, const i64 *grid3, i64 K, i64 n_classes, i64 n_taps,
                                const i64 *halo3, int form, int host, i64 workspace_bytes, i64 *out20)
{
    if (!out20 || !grid3 || !halo3) return SIT_ERR_INVALID;
    const DnPlan p = dn_plan(dn_plan_in(F, A, n_sel, frame_stride, grid3, K, n_classes, n_taps, halo3, form, host != 0, workspace_bytes),
                             sp_knobs_from_env().workspace);
    const i64 out[20] = {DN_THREADS, DN_SLOTS, DN_PROBE, p.lds_bytes, DN_RUN, p.runs, p.form, DN_TILE0, DN_TILE1, DN_TILE2,
                         p.ext[0], p.ext[1], p.ext[2], p.smooth_lds, p.window, p.n_windows, p.workspace, p.taken, p.V, p.cells};
    for (int i = 0; i < 20; i++) out20[i] = out[i];
    return p.err ? SIT_ERR_INVALID : SIT_OK;
}

static int dn_refuse(sit_ctx *c, const char *who, const char *what, i64 value, i64 limit)
{
    char text[160];
    snprintf(text, sizeof(text), "%s: %s %lld is outside [0, %lld)", who, what, (long long)value, (long long)limit);
    c->msg = text;
    return SIT_ERR_INVALID;
}

extern "C" int sit_density(sit_ctx *c, const double *positions, i64 F, i64 A, const i64 *atoms, i64 n_sel, i64 frame_stride, const i64 *grid3,
                           const int32_t *site_class, i64 K, i64 n_classes, const i64 *taps, const double *weights, i64 n_taps, int form,
                           i64 workspace_bytes, uint64_t *counts, double *smoothed, i64 *info2)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, atoms && grid3 && counts && info2, "sit_density: missing array");
    SIT_REQUIRE(c, n_taps <= 0 || (taps && weights && smoothed), "sit_density: taps without their weights or without an output");
    if (site_class) {
        SIT_SETTLE(c);
        SIT_REQUIRE(c, c->assign_valid, "sit_density: assignments needed");
        SIT_REQUIRE(c, K >= 1, "sit_density: no site");
        SIT_REQUIRE(c, F == c->F, "sit_density: F is not the number of frames of the resident labels");
        SIT_REQUIRE(c, n_sel == c->M, "sit_density: the selection is not the label columns");
        SIT_REQUIRE(c, c->assign_N == F * n_sel, "sit_density: the resident labels are not F x M");
    } else
        SIT_REQUIRE(c, K == 0 && n_classes == 1, "sit_density: classes without site_class");
    i64 halo[3] = {0, 0, 0};
    bool grid_ok = true;
    for (int a = 0; a < 3; a++) grid_ok = grid_ok && grid3[a] >= 1 && grid3[a] <= DN_MAX_GRID;
    if (grid_ok && n_taps > 0 && n_taps <= DN_MAX_TAPS)
        SIT_REQUIRE(c, dn_halo(taps, n_taps, grid3, halo), "sit_density: a tap reaches beyond (n - 1) / 2 voxels");
    const DnPlanIn in = dn_plan_in(F, A, n_sel, frame_stride, grid3, K, n_classes, n_taps, halo, form, positions != nullptr, workspace_bytes);
    const DnPlan pl = dn_plan(in, sp_knobs_from_env().workspace);
    if (pl.err) { c->msg = std::string("sit_density: ") + pl.err; return SIT_ERR_INVALID; }
    for (i64 k = 0; k < n_taps; k++) SIT_REQUIRE(c, std::isfinite(weights[k]), "sit_density: a weight is not finite");
    int rc;
    MsdCell cell;
    if ((rc = series_cell(c, "sit_density", &cell, "a degenerate cell"))) return rc;
    if (!positions && (rc = series_resident(c, "sit_density", F, A))) return rc;
    i64 bad = series_first_outside(atoms, n_sel, 0, A - 1);
    if (bad >= 0) return dn_refuse(c, "sit_density", "atom", atoms[bad], A);
    if (site_class && (bad = series_first_outside(site_class, K, 0, n_classes - 2)) >= 0)
        return dn_refuse(c, "sit_density", "class", site_class[bad], n_classes - 1);
    HIP_TRY(c, hipSetDevice(c->device));
    if (site_class && !positions) {                               // the selection is the label columns, in order
        SIT_REQUIRE(c, c->d_mobile_idx, "sit_density: the resident frames carry no mobile atoms (sit_set_frames first)");
        std::vector<i32> mobile((size_t)n_sel);
        HIP_TRY(c, hipMemcpyAsync(mobile.data(), c->d_mobile_idx, (size_t)n_sel * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (i64 i = 0; i < n_sel; i++)
            SIT_REQUIRE(c, atoms[i] == mobile[(size_t)i], "sit_density: the selection is not the label columns in order");
    }
    Scoped work(c);
    DnPieces w;
    if ((rc = carve_scratch(c, [&](Carve &cv) { w = dn_layout(cv, pl, in); }, &work))) return rc;
    HIP_TRY(c, hipMemcpyAsync(w.atoms, atoms, (size_t)n_sel * 8, hipMemcpyHostToDevice, c->stream));
    if (site_class) HIP_TRY(c, hipMemcpyAsync(w.site_class, site_class, (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    std::vector<i32> taps32((size_t)(3 * (n_taps > 0 ? n_taps : 0)));
    if (n_taps > 0) {
        for (i64 i = 0; i < 3 * n_taps; i++) taps32[(size_t)i] = (i32)taps[i];
        HIP_TRY(c, hipMemcpyAsync(w.taps, taps32.data(), (size_t)(3 * n_taps) * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(w.weights, weights, (size_t)n_taps * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemsetAsync(w.status, 0, 32, c->stream));
    HIP_TRY(c, hipMemsetAsync(w.counts, 0, (size_t)pl.cells * 8, c->stream));
    DnGrid g;
    for (int a = 0; a < 3; a++) g.n[a] = grid3[a];
    g.V = pl.V;
    const DnLabels lb = {site_class ? c->d_labels : nullptr, c->M, K, w.site_class, n_classes};
    for (i64 j0 = 0; j0 < pl.taken; j0 += pl.window) {
        const i64 nj = pl.taken - j0 < pl.window ? pl.taken - j0 : pl.window;
        SeriesSource src = {c->d_frames, A, w.atoms};
        DnRun r = {j0, nj, frame_stride, 0};
        if (positions) {
            r.f0 = j0 * frame_stride;
            const size_t bytes = (size_t)(dn_span(nj, frame_stride) * A) * 24;
            if (j0 > 0) HIP_TRY(c, hipStreamSynchronize(c->stream));      // the window before has been counted
            HIP_TRY(c, hipMemcpyAsync(w.upload, positions + r.f0 * A * 3, bytes, hipMemcpyHostToDevice, c->stream));
            src.pos = w.upload;
        }
        k_dn_count<<<dim3((unsigned)((nj + DN_RUN - 1) / DN_RUN)), dim3(DN_THREADS), 0, c->stream>>>(
            src, n_sel, r, cell, g, lb, pl.form == DN_FORM_TABLE ? 1 : 0, (u64 *)w.counts, (u64 *)w.status);
        HIP_TRY(c, hipGetLastError());
    }
    u64 *h_status = (u64 *)c->h_pinned;
    HIP_TRY(c, hipMemcpyAsync(h_status, w.status, 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = label_status(c, "sit_density", h_status[0], h_status[1], K))) return rc;
    const i64 skipped = (i64)h_status[2];
    if (n_taps > 0) {
        DnSmooth s;
        const i64 tile[3] = {DN_TILE0, DN_TILE1, DN_TILE2};
        for (int a = 0; a < 3; a++) {
            s.n[a] = grid3[a]; s.tiles[a] = (grid3[a] + tile[a] - 1) / tile[a]; s.ext[a] = (int)pl.ext[a]; s.halo[a] = (int)halo[a];
        }
        s.V = pl.V; s.n_taps = (int)n_taps; s.lds = pl.smooth_lds > 0;
        HIP_TRY(c, lds_limit((const void *)k_dn_smooth, (size_t)pl.smooth_lds, c->device));
        k_dn_smooth<<<dim3((unsigned)(s.tiles[0] * s.tiles[1] * s.tiles[2]), (unsigned)n_classes), dim3(DN_THREADS), (size_t)pl.smooth_lds,
                      c->stream>>>((const u64 *)w.counts, w.taps, w.weights, s, w.smoothed);
        HIP_TRY(c, hipGetLastError());
        if ((rc = copy_to_host(c, smoothed, w.smoothed, (size_t)pl.cells * 8))) return rc;
    }
    if ((rc = copy_to_host(c, counts, w.counts, (size_t)pl.cells * 8))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    info2[0] = pl.taken;
    info2[1] = skipped;
    return SIT_OK;
}

extern "C" int sit_density_peaks(sit_ctx *c, const double *grid, const i64 *grid3, double threshold, i64 cap, i64 *voxels, i64 *n_out)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, grid && grid3 && n_out && cap >= 0 && (voxels || cap == 0), "sit_density_peaks: missing array");
    DnGrid g;
    g.V = 1;
    for (int a = 0; a < 3; a++) {
        SIT_REQUIRE(c, grid3[a] >= 1 && grid3[a] <= DN_MAX_GRID, "sit_density_peaks: an axis of the grid holds 1 to 1024 voxels");
        g.n[a] = grid3[a]; g.V *= grid3[a];
    }
    SIT_REQUIRE(c, g.V <= DN_MAX_CELLS, "sit_density_peaks: more than 2^27 voxels");
    if (cap > g.V) cap = g.V;
    const i64 nb = (g.V + DN_THREADS - 1) / DN_THREADS;
    HIP_TRY(c, hipSetDevice(c->device));
    Scoped work(c);
    double *d_grid = nullptr; unsigned char *flag = nullptr; unsigned *block_count = nullptr; u64 *offsets = nullptr; i64 *out = nullptr;
    int rc;
    if ((rc = carve_scratch(c, [&](Carve &cv) {
            d_grid = cv.take<double>(g.V, 256);
            flag = cv.take<unsigned char>(g.V, 256);
            block_count = cv.take<unsigned>(nb, 256);
            offsets = cv.take<u64>(nb + 1, 256);
            out = cv.take<i64>(cap, 256);
        }, &work))) return rc;
    if ((rc = copy_to_device(c, d_grid, grid, (size_t)g.V * 8))) return rc;
    k_dn_peaks<<<dim3((unsigned)nb), dim3(DN_THREADS), 0, c->stream>>>(d_grid, g, threshold, flag, block_count);
    k_dn_scan<<<dim3(1), dim3(DN_THREADS), 0, c->stream>>>(block_count, nb, offsets);
    k_dn_compact<<<dim3((unsigned)nb), dim3(DN_THREADS), 0, c->stream>>>(flag, offsets, g.V, cap, out);
    HIP_TRY(c, hipGetLastError());
    u64 *h_total = (u64 *)c->h_pinned;
    HIP_TRY(c, hipMemcpyAsync(h_total, offsets + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const i64 n = (i64)h_total[0];
    *n_out = n;
    const i64 fetch = n < cap ? n : cap;
    if (fetch > 0) {
        HIP_TRY(c, hipMemcpyAsync(voxels, out, (size_t)fetch * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return SIT_OK;
}
