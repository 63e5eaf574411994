// VanHoveCorrelation / RadialDistribution: histograms of pair distances against the lag, as integer counts, from the frames
// as they lie in device memory.  Every decision - the bin of a squared distance, the image of a pair, the origins of a lag,
// the split of the pairs over workgroups, the windows and batches a workspace cap allows, the pieces of a call's buffer
// (vh_layout) - is in vanhove_plan.h; the unwrapped series of the self part are those of msd.hip (msd_series.h).
//
//   k_series_frac    (series.h, as it is) s = x . ci of the atoms of a list, per frame, as [frame][3][atom]
//   k_vh_distinct    a workgroup takes one lag, a run of origins and a span of b: each of its four waves takes an item -
//                    one origin against 64 atoms of b, a lane an atom - stages the atoms of a 64 at a time in LDS and walks
//                    them (every lane reads the same word: a broadcast); uint32 LDS counters, overflow in a register
//   k_vh_positions   y = x as [atom][3][F] (unwrap off); k_vh_self: one lag, one atom, a run of origins, a thread an origin
//   the flush        one uint64 atomic per non-zero bin of the workgroup: integer adds, the same bytes in any order
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "series.h"
#include "msd_series.h"
#include "vanhove_plan.h"
#include "sitator_hip_vanhove.h"

struct VhBins {
    const double *e2;              // [n_bins + 1]
    i64 n_bins;
    float inv_dr;
    int copies;                    // LDS histograms of a workgroup (vh_lds_bytes)
};

extern __shared__ double vh_lds[];  // vh_lds_bytes: the edges, the histograms, the tiles of k_vh_distinct

// the edges and the zeroed histograms of a workgroup; what lies behind them in LDS is the caller's
__device__ __forceinline__ double *vh_lds_begin(const VhBins &b, double *&e2s, unsigned *&hist)
{
    const i64 nb1 = b.n_bins + 1, words = nb1 * b.copies;
    e2s = vh_lds;
    hist = (unsigned *)(vh_lds + nb1);
    for (i64 i = threadIdx.x; i < nb1; i += VH_THREADS) e2s[i] = b.e2[i];
    for (i64 i = threadIdx.x; i < words; i += VH_THREADS) hist[i] = 0u;
    __syncthreads();
    return vh_lds + nb1 + (words + 1) / 2;
}

__device__ __forceinline__ void vh_count(double r2, double e2_end, const double *e2s, unsigned *mine, const VhBins &b, unsigned &over)
{
    if (r2 < e2_end) atomicAdd(&mine[vh_bin(r2, e2s, b.n_bins, vh_guess(r2, b.inv_dr))], 1u);
    else over++;
}

__device__ __forceinline__ void vh_flush(unsigned *hist, unsigned *mine, unsigned over, const VhBins &b, u64 *row)
{
    const i64 nb1 = b.n_bins + 1;
    if (over) atomicAdd(&mine[b.n_bins], over);
    __syncthreads();
    for (i64 k = threadIdx.x; k < nb1; k += VH_THREADS) {
        u64 s = 0;
        for (int cpy = 0; cpy < b.copies; cpy++) s += hist[cpy * nb1 + k];
        if (s) atomicAdd(&row[k], s);
    }
}

struct VhDistinct {
    const double *sa, *sb;         // [frames held][3][n_a], [frames held][3][n_b]
    i64 fa0, fb0;                  // the frame the first one held is
    i64 o_begin, o_end;            // origins of this launch, by number: t = o * stride
    const i64 *lags;               // [grid.y]
    i64 F, stride, n_a, n_b, run, b_span;
    int same;
    u64 *counts;                   // [grid.y][n_bins + 1]
};

__global__ __launch_bounds__(VH_THREADS) void k_vh_distinct(VhDistinct g, VhBins bins, MsdCell cell)
{
    const i64 tau = g.lags[blockIdx.y];
    const i64 n_or = series_origins(g.F, tau, g.stride);
    i64 o_hi = g.o_end < n_or ? g.o_end : n_or;
    const i64 o_lo = g.o_begin + (i64)blockIdx.x * g.run;
    if (o_lo >= o_hi) return;                                    // the whole workgroup
    if (o_lo + g.run < o_hi) o_hi = o_lo + g.run;
    double *e2s; unsigned *hist;
    double *tile = vh_lds_begin(bins, e2s, hist);
    const int wave = threadIdx.x / VH_WAVE, lane = threadIdx.x % VH_WAVE;
    double *ta = tile + wave * 3 * VH_WAVE;
    unsigned *mine = hist + (bins.copies > 1 ? wave * (bins.n_bins + 1) : 0);
    const double e2_end = e2s[bins.n_bins];
    const i64 b_lo = (i64)blockIdx.z * g.b_span, b_hi = b_lo + g.b_span < g.n_b ? b_lo + g.b_span : g.n_b;
    const i64 chunks = (b_hi - b_lo + VH_WAVE - 1) / VH_WAVE, items = (o_hi - o_lo) * chunks;
    unsigned over = 0;
    for (i64 base = 0; base < items; base += VH_WAVES) {         // the same trips for every wave: the barriers below
        const i64 item = base + wave;
        const bool live = item < items;
        const i64 o = o_lo + item / chunks, b = b_lo + (item % chunks) * VH_WAVE + lane;
        const bool has_b = live && b < b_hi;
        const double *pa = g.sa;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (live) {
            const i64 t = o * g.stride;
            pa = g.sa + (t - g.fa0) * 3 * g.n_a;
            if (has_b) {
                const double *pb = g.sb + (t + tau - g.fb0) * 3 * g.n_b;
                s0 = pb[b]; s1 = pb[g.n_b + b]; s2 = pb[2 * g.n_b + b];
            }
        }
        for (i64 a0 = 0; a0 < g.n_a; a0 += VH_WAVE) {
            __syncthreads();                                     // the tile before has been walked
            if (live && a0 + lane < g.n_a) {
                ta[lane] = pa[a0 + lane]; ta[VH_WAVE + lane] = pa[g.n_a + a0 + lane]; ta[2 * VH_WAVE + lane] = pa[2 * g.n_a + a0 + lane];
            }
            __syncthreads();
            if (!has_b) continue;
            const int n = g.n_a - a0 < VH_WAVE ? (int)(g.n_a - a0) : VH_WAVE;
            const i64 skip = g.same ? b - a0 : -1;               // the pair of equal position in the two lists
            for (int j = 0; j < n; j++) {
                if (j == skip) continue;
                vh_count(vh_image_r2(s0 - ta[j], s1 - ta[VH_WAVE + j], s2 - ta[2 * VH_WAVE + j], cell.cm), e2_end, e2s, mine, bins, over);
            }
        }
    }
    vh_flush(hist, mine, over, bins, g.counts + (i64)blockIdx.y * (bins.n_bins + 1));
}

// y[c][a][t] = x: the positions as they are, through the tile of series.h
__global__ __launch_bounds__(256) void k_vh_positions(SeriesSource src, i64 a0, i64 nb, i64 F, double *y)
{
    series_tile<3, double>(a0, nb, F,
        [&](i64 t, i64 column, double *x) { const double *p = src.at(t, column); x[0] = p[0]; x[1] = p[1]; x[2] = p[2]; },
        [&](i64 t, i64 c, const double *x) { for (int a = 0; a < 3; a++) y[(c * 3 + a) * F + t] = x[a]; });
}

// grid: (runs of VH_SELF_RUN origins, lags, atoms of the batch); y [atom][3][F]
__global__ __launch_bounds__(VH_THREADS) void k_vh_self(const double *y, i64 F, i64 stride, const i64 *lags, VhBins bins, u64 *counts)
{
    const i64 tau = lags[blockIdx.y];
    const i64 n_or = series_origins(F, tau, stride);
    const i64 o_lo = (i64)blockIdx.x * VH_SELF_RUN;
    if (o_lo >= n_or) return;
    const i64 o_hi = o_lo + VH_SELF_RUN < n_or ? o_lo + VH_SELF_RUN : n_or;
    double *e2s; unsigned *hist;
    vh_lds_begin(bins, e2s, hist);
    unsigned *mine = hist + (bins.copies > 1 ? (threadIdx.x / VH_WAVE) * (bins.n_bins + 1) : 0);
    const double e2_end = e2s[bins.n_bins];
    const double *yx = y + (i64)blockIdx.z * 3 * F, *yy = yx + F, *yz = yy + F;
    unsigned over = 0;
    for (i64 o = o_lo + threadIdx.x; o < o_hi; o += VH_THREADS) {
        const i64 t = o * stride;
        vh_count(vh_r2(yx[t + tau] - yx[t], yy[t + tau] - yy[t], yz[t + tau] - yz[t]), e2_end, e2s, mine, bins, over);
    }
    vh_flush(hist, mine, over, bins, counts + (i64)blockIdx.y * (bins.n_bins + 1));
}

// ---- host side ------------------------------------------------------------------------------------------------------------

// SITATOR_VANHOVE_HIST_COPIES=4: one LDS histogram per wave instead of one per workgroup (DESIGN.md section 21 has both timings)
static int vh_hist_copies()
{
    const char *e = getenv("SITATOR_VANHOVE_HIST_COPIES");
    return e && atoi(e) == VH_WAVES ? VH_WAVES : 1;
}

static VhPlanIn vh_plan_in(i64 F, i64 n_a, i64 n_b, i64 n_lags, i64 n_bins, i64 stride, bool self_part, bool distinct_part, bool unwrap,
                           i64 workspace_bytes)
{
    VhPlanIn in;
    in.F = F; in.n_a = n_a; in.n_b = n_b; in.n_lags = n_lags; in.n_bins = n_bins; in.stride = stride;
    in.want_self = self_part; in.want_distinct = distinct_part; in.unwrap = unwrap; in.workspace_bytes = workspace_bytes;
    in.hist_copies = vh_hist_copies();
    return in;
}

extern "C" int sit_vanhove_plan(i64 F, i64 n_a, i64 n_b, i64 n_lags, i64 n_bins, i64 origin_stride, int self_part, int distinct_part,
                                int unwrap, i64 workspace_bytes, i64 *out12)
{
    if (!out12 || workspace_bytes < 0) return SIT_ERR_INVALID;
    const VhPlan p = vh_plan(vh_plan_in(F, n_a, n_b, n_lags, n_bins, origin_stride, self_part != 0, distinct_part != 0, unwrap != 0, workspace_bytes),
                             sp_knobs_from_env().workspace);
    const i64 out[12] = {VH_THREADS, VH_MAX_BINS, VH_MAX_ATOMS, p.run, p.b_span, p.pairs_per_wg, p.b_tiles, p.window, p.self_batch,
                         p.lds_bytes, p.workspace, VH_SELF_RUN};
    for (int i = 0; i < 12; i++) out12[i] = out[i];
    return p.err ? SIT_ERR_INVALID : SIT_OK;
}

extern "C" int sit_vanhove(sit_ctx *c, const double *positions, i64 F, i64 A, const i64 *atoms_a, i64 n_a, const i64 *atoms_b, i64 n_b,
                           int same, const i64 *lags, i64 n_lags, i64 origin_stride, double r_max, i64 n_bins, int unwrap,
                           i64 workspace_bytes, uint64_t *self_counts, uint64_t *distinct_counts, double *max_residual)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, self_counts || distinct_counts, "sit_vanhove: both outputs are NULL");
    SIT_REQUIRE(c, atoms_a && atoms_b && lags, "sit_vanhove: missing array");
    SIT_REQUIRE(c, workspace_bytes >= 0, "sit_vanhove: negative count");
    SIT_REQUIRE(c, !same || n_a == n_b, "sit_vanhove: one selection in two lists of different lengths");
    if (max_residual) *max_residual = 0.0;
    const VhPlanIn in = vh_plan_in(F, n_a, n_b, n_lags, n_bins, origin_stride, self_counts != nullptr, distinct_counts != nullptr, unwrap != 0,
                                   workspace_bytes);
    const VhPlan pl = vh_plan(in, sp_knobs_from_env().workspace);
    if (pl.err) { c->msg = std::string("sit_vanhove: ") + pl.err; return SIT_ERR_INVALID; }
    int rc;
    MsdCell cell;
    if ((rc = series_lags(c, "sit_vanhove", lags, n_lags, F)) || (rc = series_cell(c, "sit_vanhove", &cell, "a degenerate cell"))) return rc;
    SIT_REQUIRE(c, vh_rmax_ok(r_max, vh_hmin(cell.ci)), "sit_vanhove: r_max is outside (0, hmin / 2 (1 - 2^-30)] of the cell");
    if (!positions && (rc = series_resident(c, "sit_vanhove", F, A))) return rc;
    SIT_REQUIRE(c, A >= 1, "sit_vanhove: no atom in a frame");
    if ((rc = series_atoms_in_range(c, "sit_vanhove", atoms_a, n_a, A)) || (rc = series_atoms_in_range(c, "sit_vanhove", atoms_b, n_b, A))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    Scoped work(c), upload(c);
    VhPieces w;
    if ((rc = carve_scratch(c, [&](Carve &cv) { w = vh_layout(cv, pl, in); }, &work))) return rc;
    const i64 nb1 = n_bins + 1, table = n_lags * nb1;
    std::vector<double> e2((size_t)nb1);
    vh_edges2(r_max, n_bins, e2.data());
    HIP_TRY(c, hipMemsetAsync(w.status, 0, 8, c->stream));
    if (self_counts) HIP_TRY(c, hipMemsetAsync(w.self_counts, 0, (size_t)table * 8, c->stream));
    if (distinct_counts) HIP_TRY(c, hipMemsetAsync(w.distinct_counts, 0, (size_t)table * 8, c->stream));
    HIP_TRY(c, hipMemcpyAsync(w.atoms, atoms_a, (size_t)n_a * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(w.atoms + n_a, atoms_b, (size_t)n_b * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(w.lags, lags, (size_t)n_lags * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(w.e2, e2.data(), (size_t)nb1 * 8, hipMemcpyHostToDevice, c->stream));
    SeriesSource src;
    if ((rc = series_frames(c, positions, F, A, w.atoms, upload, &src))) return rc;
    VhBins bins;
    bins.e2 = w.e2; bins.n_bins = n_bins; bins.inv_dr = (float)((double)n_bins / r_max); bins.copies = in.hist_copies;
    const size_t lds = (size_t)pl.lds_bytes;
    const i64 most_origins = series_origins(F, 0, origin_stride);
    if (distinct_counts) {
        HIP_TRY(c, lds_limit((const void *)k_vh_distinct, lds, c->device));
        VhDistinct g;
        g.sa = w.sa; g.sb = w.sb; g.F = F; g.stride = origin_stride; g.n_a = n_a; g.n_b = n_b; g.run = pl.run; g.b_span = pl.b_span;
        g.same = same != 0;
        const auto launch = [&](i64 l0, i64 nl) -> int {
            const i64 runs = (g.o_end - g.o_begin + pl.run - 1) / pl.run;
            g.lags = w.lags + l0; g.counts = w.distinct_counts + l0 * nb1;
            k_vh_distinct<<<dim3((unsigned)runs, (unsigned)nl, (unsigned)pl.b_tiles), dim3(VH_THREADS), lds, c->stream>>>(g, bins, cell);
            HIP_TRY(c, hipGetLastError());
            return SIT_OK;
        };
        if (pl.window >= F) {                                    // every frame held: all lags at once
            if ((rc = series_frac(c, src, 0, n_a, 0, F, cell, w.sa)) || (rc = series_frac(c, src, n_a, n_b, 0, F, cell, w.sb))) return rc;
            g.fa0 = g.fb0 = 0; g.o_begin = 0; g.o_end = most_origins;
            for (i64 l0 = 0; l0 < n_lags; l0 += VH_MAX_GRID_YZ)
                if ((rc = launch(l0, n_lags - l0 < VH_MAX_GRID_YZ ? n_lags - l0 : VH_MAX_GRID_YZ))) return rc;
        } else {
            // a lag at a time: the frames of a window of origins for a, the same frames a lag later for b
            for (i64 l = 0; l < n_lags; l++) {
                const i64 tau = lags[l], n_or = series_origins(F, tau, origin_stride);
                for (i64 o0 = 0; o0 < n_or; o0 += pl.origins_per_window) {
                    const i64 o1 = o0 + pl.origins_per_window < n_or ? o0 + pl.origins_per_window : n_or;
                    const i64 f0 = o0 * origin_stride, nf = (o1 - 1) * origin_stride - f0 + 1;
                    if ((rc = series_frac(c, src, 0, n_a, f0, nf, cell, w.sa)) || (rc = series_frac(c, src, n_a, n_b, f0 + tau, nf, cell, w.sb))) return rc;
                    g.fa0 = f0; g.fb0 = f0 + tau; g.o_begin = o0; g.o_end = o1;
                    if ((rc = launch(l, 1))) return rc;
                }
            }
        }
    }
    if (self_counts) {
        HIP_TRY(c, lds_limit((const void *)k_vh_self, lds, c->device));
        const i64 B = pl.self_batch;
        for (i64 a0 = 0; a0 < n_a; a0 += B) {
            const i64 nb = a0 + B < n_a ? B : n_a - a0;
            if (unwrap) {
                if ((rc = msd_series_launch(c, src, a0, nb, F, cell, true, pl.n_chunks, w.images, w.totals, w.y, w.status))) return rc;
            } else {
                k_vh_positions<<<dim3((unsigned)((F + 31) / 32), (unsigned)((nb + 31) / 32)), dim3(256), 0, c->stream>>>(src, a0, nb, F, w.y);
                HIP_TRY(c, hipGetLastError());
            }
            const i64 runs = (most_origins + VH_SELF_RUN - 1) / VH_SELF_RUN;
            for (i64 l0 = 0; l0 < n_lags; l0 += VH_MAX_GRID_YZ) {
                const i64 nl = n_lags - l0 < VH_MAX_GRID_YZ ? n_lags - l0 : VH_MAX_GRID_YZ;
                k_vh_self<<<dim3((unsigned)runs, (unsigned)nl, (unsigned)nb), dim3(VH_THREADS), lds, c->stream>>>(
                    w.y, F, origin_stride, w.lags + l0, bins, w.self_counts + l0 * nb1);
                HIP_TRY(c, hipGetLastError());
            }
        }
    }
    u64 bits = 0;
    if (self_counts) HIP_TRY(c, hipMemcpyAsync(self_counts, w.self_counts, (size_t)table * 8, hipMemcpyDeviceToHost, c->stream));
    if (distinct_counts) HIP_TRY(c, hipMemcpyAsync(distinct_counts, w.distinct_counts, (size_t)table * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&bits, w.status, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (max_residual) { double v; memcpy(&v, &bits, 8); *max_residual = v; }
    return SIT_OK;
}
