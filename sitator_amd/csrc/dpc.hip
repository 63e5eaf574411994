// SiteTypeAnalysis on the device (site_descriptors/SiteTypeAnalysis.py:83-156): the PCA statistics and projection, and
// density-peak clustering without the N x N matrix pydpc keeps.  Every decision is in dpc_plan.h (the host compiler builds it too);
// here are the kernels and the entry points.  Distances are recomputed wherever they are needed: the point of a thread lies in
// registers, the points it is compared with stream through LDS a tile at a time.
#include <algorithm>

#include "sit_internal.h"
#include "dpc_plan.h"

#define PC_ROWS 1024                                   // rows of a chunk of the PCA sums
#define PC_EDGE 16                                     // a workgroup of the covariance takes a 16 x 16 block of entries
#define PC_MAX_D 4096
#define PC_MAX_N 33554432                              // 2^25 rows: 32768 chunks (grid.z)
#define PC_MAX_PARTIAL ((i64)8 << 30)                  // bytes of the per-chunk covariance sums

__host__ __device__ static inline i64 imin64(i64 a, i64 b) { return a < b ? a : b; }

// ---- density-peak clustering ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(DP_BLOCK) void k_dpc_pad(const double *Y, i64 N, int D, int DPp, double *Yp, unsigned *status)
{
    const i64 idx = (i64)blockIdx.x * DP_BLOCK + threadIdx.x;
    if (idx >= N * DPp) return;
    const i64 r = idx / DPp;
    const int k = (int)(idx - r * DPp);
    const double v = k < D ? Y[r * D + k] : 0.0;
    if (!(fabs(v) <= DP_MAX_ABS)) atomicOr(status, 1u);            // NaN fails the comparison too
    Yp[idx] = v;
}

template <int DPp> __device__ __forceinline__ void dpc_stage(double *tile, const double *Yp, i64 t, i64 N)
{
    const i64 base = t * DP_TILE * DPp, end = N * DPp;
    for (int q = threadIdx.x; q < DP_TILE * DPp; q += DP_BLOCK) {
        const i64 g = base + q;
        tile[q] = g < end ? Yp[g] : 0.0;
    }
}

template <int DPp> __device__ __forceinline__ void dpc_own(double *yi, const double *Yp, i64 i, i64 N)
{
#pragma unroll
    for (int k = 0; k < DPp; k++) yi[k] = i < N ? Yp[i * DPp + k] : 0.0;
}

// one pass of the radix select over the pairs of tiles (dp_tile_pair): LDS counts, flushed with integer atomics
template <int DPp>
__global__ __launch_bounds__(DP_BLOCK) void k_dpc_hist(const double *Yp, i64 N, i64 T, int pass, u64 prefix, u64 *hist)
{
    extern __shared__ double dpc_smem[];
    double *tile = dpc_smem;
    unsigned *h = (unsigned *)(dpc_smem + DP_TILE * DPp);
    i64 lo, hi;
    if (!dp_tile_pair(blockIdx.x, blockIdx.y, T, &lo, &hi)) return;
    const i64 i = lo * DP_TILE + threadIdx.x;
    double yi[DPp];
    dpc_own<DPp>(yi, Yp, i, N);
    h[threadIdx.x] = 0;
    dpc_stage<DPp>(tile, Yp, hi, N);
    __syncthreads();
    const i64 j0 = hi * DP_TILE;
    const int nj = (int)imin64(DP_TILE, N - j0);
    // a thread's distances mostly fall into one count (all of them in the first passes, hardly any later): runs are added at once
    int cur = -1;
    unsigned run = 0;
    for (int jj = 0; jj < nj; jj++) {
        const i64 j = j0 + jj;
        const u64 bits = dp_bits(dp_dist<DPp>(yi, tile + jj * DPp));
        if (i < j && i < N && dp_match(bits, pass, prefix)) {
            const int g = dp_digit(bits, pass);
            if (g != cur) {
                if (run) atomicAdd(&h[cur], run);
                cur = g; run = 0;
            }
            run++;
        }
    }
    if (run) atomicAdd(&h[cur], run);
    __syncthreads();
    const unsigned mine = h[threadIdx.x];                          // at most 65536 pairs of a workgroup
    if (mine) atomicAdd(&hist[threadIdx.x], (u64)mine);
}

// the terms of segment blockIdx.y for the points of tile blockIdx.x, in ascending j
template <int DPp>
__global__ __launch_bounds__(DP_BLOCK) void k_dpc_rho(const double *Yp, i64 N, i64 T, double dc, double *partial)
{
    extern __shared__ double dpc_smem[];
    double *tile = dpc_smem;
    const i64 i = (i64)blockIdx.x * DP_TILE + threadIdx.x;
    double yi[DPp];
    dpc_own<DPp>(yi, Yp, i, N);
    i64 first, last;
    dp_segment(T, (int)blockIdx.y, &first, &last);
    double acc = 0.0;
    for (i64 t = first; t < last; t++) {
        __syncthreads();
        dpc_stage<DPp>(tile, Yp, t, N);
        __syncthreads();
        const i64 j0 = t * DP_TILE;
        const int nj = (int)imin64(DP_TILE, N - j0);
        for (int jj = 0; jj < nj; jj++) {
            const double d = dp_dist<DPp>(yi, tile + jj * DPp);
            if (j0 + jj != i) acc = acc + dp_weight(d, dc);
        }
    }
    if (i < N) partial[(i64)blockIdx.y * N + i] = acc;
}

__global__ __launch_bounds__(DP_BLOCK) void k_dpc_rho_sum(const double *partial, i64 N, double *rho)
{
    const i64 i = (i64)blockIdx.x * DP_BLOCK + threadIdx.x;
    if (i >= N) return;
    double s = partial[i];
    for (int q = 1; q < DP_SPLIT; q++) s = s + partial[(i64)q * N + i];
    rho[i] = s;
}

// the nearest point above i within segment blockIdx.y
template <int DPp>
__global__ __launch_bounds__(DP_BLOCK) void k_dpc_delta(const double *Yp, const double *rho, i64 N, i64 T, double *pd, i32 *pj)
{
    extern __shared__ double dpc_smem[];
    double *tile = dpc_smem;
    double *rt = dpc_smem + DP_TILE * DPp;
    const i64 i = (i64)blockIdx.x * DP_TILE + threadIdx.x;
    double yi[DPp];
    dpc_own<DPp>(yi, Yp, i, N);
    const double rho_i = i < N ? rho[i] : 0.0;
    i64 first, last;
    dp_segment(T, (int)blockIdx.y, &first, &last);
    double best_d = 0.0, best_rho = 0.0;
    i64 best_j = -1;
    for (i64 t = first; t < last; t++) {
        __syncthreads();
        dpc_stage<DPp>(tile, Yp, t, N);
        const i64 j0 = t * DP_TILE;
        rt[threadIdx.x] = j0 + threadIdx.x < N ? rho[j0 + threadIdx.x] : 0.0;
        __syncthreads();
        const int nj = (int)imin64(DP_TILE, N - j0);
        for (int jj = 0; jj < nj; jj++) {
            const i64 j = j0 + jj;
            const double rho_j = rt[jj];
            if (j == i || !dp_above(rho_j, j, rho_i, i)) continue;
            const double d = dp_dist<DPp>(yi, tile + jj * DPp);
            if (dp_better(d, rho_j, j, best_d, best_rho, best_j)) { best_d = d; best_rho = rho_j; best_j = j; }
        }
    }
    if (i < N) {
        pd[(i64)blockIdx.y * N + i] = best_d;
        pj[(i64)blockIdx.y * N + i] = (i32)best_j;
    }
}

// words: [0] the largest delta as its bit pattern (non-negative doubles order as their bits), [1] the top point + 1
__global__ __launch_bounds__(DP_BLOCK) void k_dpc_delta_fin(const double *pd, const i32 *pj, const double *rho, i64 N, double *delta,
                                                            i32 *neighbour, u64 *words)
{
    const i64 i = (i64)blockIdx.x * DP_BLOCK + threadIdx.x;
    if (i >= N) return;
    double best_d = 0.0, best_rho = 0.0;
    i64 best_j = -1;
    for (int q = 0; q < DP_SPLIT; q++) {
        const i64 j = pj[(i64)q * N + i];
        if (j < 0 || j >= N) continue;
        const double d = pd[(i64)q * N + i], rho_j = rho[j];
        if (dp_better(d, rho_j, j, best_d, best_rho, best_j)) { best_d = d; best_rho = rho_j; best_j = j; }
    }
    neighbour[i] = (i32)best_j;
    delta[i] = best_d;
    if (best_j < 0) words[1] = (u64)(i + 1);
    else atomicMax(&words[0], dp_bits(best_d));
}

__global__ void k_dpc_top(double *delta, i64 N, const u64 *words)
{
    const u64 top = words[1];
    if (threadIdx.x == 0 && blockIdx.x == 0 && top >= 1 && top <= (u64)N) delta[top - 1] = dp_from_bits(words[0]);
}

// membership: the starting pointers, the rounds, the numbers, the votes
__global__ __launch_bounds__(DP_BLOCK) void k_dpc_start(const i32 *cid, const i32 *neighbour, i64 N, i32 *p)
{
    const i64 i = (i64)blockIdx.x * DP_BLOCK + threadIdx.x;
    if (i < N) p[i] = dp_start((i32)i, cid[i] >= 0, neighbour[i]);
}

__global__ __launch_bounds__(DP_BLOCK) void k_dpc_jump(const i32 *p, i32 *next, i64 N, unsigned *changed)
{
    const i64 i = (i64)blockIdx.x * DP_BLOCK + threadIdx.x;
    if (i >= N) return;
    const i32 a = p[i];
    const i32 b = (a >= 0 && a < N) ? p[a] : a;
    next[i] = b;
    if (b != a) *changed = 1u;
}

__global__ __launch_bounds__(DP_BLOCK) void k_dpc_member(const i32 *p, const i32 *cid, const i64 *site, i64 N, i64 n_clusters, i32 *membership,
                                                         u64 *votes)
{
    const i64 i = (i64)blockIdx.x * DP_BLOCK + threadIdx.x;
    if (i >= N) return;
    const i32 a = p[i];
    const i32 m = (a >= 0 && a < N) ? cid[a] : -1;
    membership[i] = m;
    if (votes && m >= 0 && m < n_clusters) atomicAdd(&votes[site[i] * n_clusters + m], 1ull);
}

static int dpc_lds(sit_ctx *c, int DPp)
{
    const size_t bytes = (size_t)dp_lds_bytes(DPp);
#define DPC_LDS_CASE(P)                                                                                                         \
    case P:                                                                                                                     \
        HIP_TRY(c, lds_limit((const void *)k_dpc_hist<P>, bytes, c->device));                                                   \
        HIP_TRY(c, lds_limit((const void *)k_dpc_rho<P>, bytes, c->device));                                                    \
        HIP_TRY(c, lds_limit((const void *)k_dpc_delta<P>, bytes, c->device));                                                  \
        break;
    switch (DPp) { DPC_LDS_CASE(2) DPC_LDS_CASE(4) DPC_LDS_CASE(8) DPC_LDS_CASE(16) DPC_LDS_CASE(32) }
#undef DPC_LDS_CASE
    return SIT_OK;
}

#define DPC_LAUNCH(DPp, kernel, grid, lds, stream, ...)                                                                         \
    switch (DPp) {                                                                                                              \
    case 2: kernel<2><<<grid, dim3(DP_BLOCK), lds, stream>>>(__VA_ARGS__); break;                                               \
    case 4: kernel<4><<<grid, dim3(DP_BLOCK), lds, stream>>>(__VA_ARGS__); break;                                               \
    case 8: kernel<8><<<grid, dim3(DP_BLOCK), lds, stream>>>(__VA_ARGS__); break;                                               \
    case 16: kernel<16><<<grid, dim3(DP_BLOCK), lds, stream>>>(__VA_ARGS__); break;                                             \
    default: kernel<32><<<grid, dim3(DP_BLOCK), lds, stream>>>(__VA_ARGS__); break;                                             \
    }

static inline unsigned dpc_blocks(i64 n) { return (unsigned)((n + DP_BLOCK - 1) / DP_BLOCK); }

extern "C" int sit_dpc_plan(i64 d, i64 *out12)
{
    if (!out12) return SIT_ERR_INVALID;
    out12[0] = DP_BLOCK; out12[1] = DP_TILE; out12[2] = DP_DIGIT_BITS; out12[3] = DP_PASSES; out12[4] = DP_MAX_D; out12[5] = 0;
    out12[6] = DP_SPLIT; out12[7] = DP_MAX_N; out12[8] = PC_ROWS; out12[9] = PC_EDGE; out12[10] = PC_MAX_D; out12[11] = PC_MAX_N;
    if (d < 1) return SIT_ERR_INVALID;
    if (d > DP_MAX_D) return SIT_ERR_CAPACITY;
    out12[5] = dp_lds_bytes((int)d);
    return SIT_OK;
}

extern "C" int sit_dpc_graph(sit_ctx *c, const double *Y, i64 N, i64 d, double fraction, double *kernel_size, double *density, double *delta,
                             i32 *neighbour, double *info2)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    bool invalid;
    const int what = dp_check(N, d, fraction, &invalid);
    if (what) {
        c->msg = std::string("sit_dpc_graph: ") + dp_limit_text(what);
        return invalid ? SIT_ERR_INVALID : SIT_ERR_CAPACITY;
    }
    SIT_REQUIRE(c, Y && kernel_size && density && delta && neighbour, "sit_dpc_graph: missing array");
    HIP_TRY(c, hipSetDevice(c->device));
    const int D = (int)d, DPp = dp_padded(D);
    const i64 T = dp_tiles(N), n = dp_pairs(N);
    const size_t lds = (size_t)dp_lds_bytes(D);

    u64 *d_hist, *d_words;
    unsigned *d_status;
    int rc = carve_scratch(c, [&](Carve &cv) {
        d_hist = cv.take<u64>(DP_BINS, 64); d_words = cv.take<u64>(8, 64); d_status = cv.take<unsigned>(16, 64);
    });
    if (rc) return rc;
    double *d_raw, *d_Yp, *d_part, *d_rho, *d_delta;
    i32 *d_pj, *d_nbr;
    auto lay = [&](Carve &cv) {
        d_Yp = cv.take<double>(N * DPp, 256); d_part = cv.take<double>(N * DP_SPLIT, 256); d_rho = cv.take<double>(N, 256);
        d_delta = cv.take<double>(N, 256); d_pj = cv.take<i32>(N * DP_SPLIT, 256); d_nbr = cv.take<i32>(N, 256);
        d_raw = cv.take<double>(N * D, 256);
    };
    Carve cv = {nullptr, 0};
    lay(cv);
    Scoped buf(c);
    HIP_TRY(c, sit_dmalloc(c, &buf.p, (size_t)cv.used));
    cv = {(char *)buf.p, 0};
    lay(cv);
    if ((rc = dpc_lds(c, DPp))) return rc;
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    HIP_TRY(c, hipEventCreate(&ev.e0));
    HIP_TRY(c, hipEventCreate(&ev.e1));

    if ((rc = copy_to_device(c, d_raw, Y, (size_t)(N * D) * 8))) return rc;
    HIP_TRY(c, hipMemsetAsync(d_status, 0, 64, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_words, 0, 64, c->stream));
    HIP_TRY(c, hipEventRecord(ev.e0, c->stream));
    k_dpc_pad<<<dim3(dpc_blocks(N * DPp)), dim3(DP_BLOCK), 0, c->stream>>>(d_raw, N, D, DPp, d_Yp, d_status);
    HIP_TRY(c, hipGetLastError());
    unsigned *h_status = (unsigned *)c->h_pinned;
    HIP_TRY(c, hipMemcpyAsync(h_status, d_status, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    SIT_REQUIRE(c, h_status[0] == 0, "sit_dpc_graph: a coordinate that is not finite or beyond 1e150");

    // the kernel size: eight counting passes, the digit chosen on the host in between
    const dim3 pair_grid((unsigned)T, (unsigned)(T / 2 + 1));
    std::vector<uint64_t> hist(DP_BINS);
    uint64_t prefix = 0;
    int64_t rank = dp_rank(n, fraction);
    for (int pass = 0; pass < DP_PASSES; pass++) {
        HIP_TRY(c, hipMemsetAsync(d_hist, 0, DP_BINS * 8, c->stream));
        DPC_LAUNCH(DPp, k_dpc_hist, pair_grid, lds, c->stream, d_Yp, N, T, pass, (u64)prefix, d_hist);
        HIP_TRY(c, hipGetLastError());
        if ((rc = copy_to_host(c, hist.data(), d_hist, DP_BINS * 8))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!dp_select_step(hist.data(), &prefix, &rank)) {
            c->msg = "sit_dpc_graph: a pass of the select counted fewer distances than the rank asks for";
            return SIT_ERR_HIP;
        }
    }
    const double dc = dp_from_bits(prefix);

    const dim3 seg_grid((unsigned)T, DP_SPLIT);
    DPC_LAUNCH(DPp, k_dpc_rho, seg_grid, lds, c->stream, d_Yp, N, T, dc, d_part);
    k_dpc_rho_sum<<<dim3(dpc_blocks(N)), dim3(DP_BLOCK), 0, c->stream>>>(d_part, N, d_rho);
    DPC_LAUNCH(DPp, k_dpc_delta, seg_grid, lds, c->stream, d_Yp, d_rho, N, T, d_part, d_pj);
    k_dpc_delta_fin<<<dim3(dpc_blocks(N)), dim3(DP_BLOCK), 0, c->stream>>>(d_part, d_pj, d_rho, N, d_delta, d_nbr, d_words);
    k_dpc_top<<<dim3(1), dim3(64), 0, c->stream>>>(d_delta, N, d_words);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(ev.e1, c->stream));
    if ((rc = copy_to_host(c, density, d_rho, (size_t)N * 8))) return rc;
    if ((rc = copy_to_host(c, delta, d_delta, (size_t)N * 8))) return rc;
    if ((rc = copy_to_host(c, neighbour, d_nbr, (size_t)N * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *kernel_size = dc;
    if (info2) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
        info2[0] = ms; info2[1] = (double)n;
    }
    return SIT_OK;
}

extern "C" int sit_dpc_assign(sit_ctx *c, const double *density, const double *delta, const i32 *neighbour, i64 N, double min_density,
                              double min_delta, const i64 *dvecs_to_site, i64 K, i32 *membership, i32 *clusters, i64 *n_clusters,
                              i64 *votes, i64 votes_cap)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, N >= 2, "sit_dpc_assign: fewer than 2 points");
    if (N > DP_MAX_N) { c->msg = std::string("sit_dpc_assign: ") + dp_limit_text(5); return SIT_ERR_CAPACITY; }
    SIT_REQUIRE(c, density && delta && neighbour && membership && clusters && n_clusters, "sit_dpc_assign: missing array");
    SIT_REQUIRE(c, K >= 0 && (K == 0 || dvecs_to_site), "sit_dpc_assign: K sites need dvecs_to_site");
    SIT_REQUIRE(c, min_density == min_density && min_delta == min_delta, "sit_dpc_assign: a threshold that is not a number");
    // the centres, numbered in ascending index (the list is an output; the rule is dpc_plan.h's)
    std::vector<i32> cid((size_t)N);
    i64 nc = 0;
    for (i64 i = 0; i < N; i++) {
        SIT_REQUIRE(c, fabs(density[i]) < INFINITY && fabs(delta[i]) < INFINITY, "sit_dpc_assign: a density or delta that is not finite");
        SIT_REQUIRE(c, neighbour[i] >= -1 && neighbour[i] < N, "sit_dpc_assign: a neighbour outside [-1, N)");
        if (K > 0 && (dvecs_to_site[i] < 0 || dvecs_to_site[i] >= K)) return index_out_of_bounds(c, dvecs_to_site[i], K);
        const bool centre = dp_is_centre(density[i], delta[i], min_density, min_delta);
        cid[(size_t)i] = centre ? (i32)nc : -1;
        if (centre) clusters[nc++] = (i32)i;
    }
    *n_clusters = nc;
    const bool vote = votes && K > 0 && nc > 0 && K * nc <= votes_cap;
    HIP_TRY(c, hipSetDevice(c->device));

    unsigned *d_changed;
    int rc = carve_scratch(c, [&](Carve &cv) { d_changed = cv.take<unsigned>(16, 64); });
    if (rc) return rc;
    i32 *d_cid, *d_nbr, *d_p, *d_q, *d_member;
    i64 *d_site;
    u64 *d_votes;
    auto lay = [&](Carve &cv) {
        d_cid = cv.take<i32>(N, 256); d_nbr = cv.take<i32>(N, 256); d_p = cv.take<i32>(N, 256); d_q = cv.take<i32>(N, 256);
        d_member = cv.take<i32>(N, 256); d_site = cv.take<i64>(vote ? N : 0, 256); d_votes = cv.take<u64>(vote ? K * nc : 0, 256);
    };
    Carve cv = {nullptr, 0};
    lay(cv);
    Scoped buf(c);
    HIP_TRY(c, sit_dmalloc(c, &buf.p, (size_t)cv.used));
    cv = {(char *)buf.p, 0};
    lay(cv);
    if ((rc = copy_to_device(c, d_cid, cid.data(), (size_t)N * 4))) return rc;
    if ((rc = copy_to_device(c, d_nbr, neighbour, (size_t)N * 4))) return rc;
    if (vote) {
        if ((rc = copy_to_device(c, d_site, dvecs_to_site, (size_t)N * 8))) return rc;
        HIP_TRY(c, hipMemsetAsync(d_votes, 0, (size_t)(K * nc) * 8, c->stream));
    }
    const dim3 grid(dpc_blocks(N));
    k_dpc_start<<<grid, dim3(DP_BLOCK), 0, c->stream>>>(d_cid, d_nbr, N, d_p);
    HIP_TRY(c, hipGetLastError());
    unsigned *h_changed = (unsigned *)c->h_pinned;
    bool settled = false;
    for (int round = 0; round < DP_MAX_ROUNDS && !settled; round++) {
        HIP_TRY(c, hipMemsetAsync(d_changed, 0, 4, c->stream));
        k_dpc_jump<<<grid, dim3(DP_BLOCK), 0, c->stream>>>(d_p, d_q, N, d_changed);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h_changed, d_changed, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::swap(d_p, d_q);
        settled = h_changed[0] == 0;
    }
    SIT_REQUIRE(c, settled, "sit_dpc_assign: the neighbours do not form a forest (a chain came back to itself)");
    k_dpc_member<<<grid, dim3(DP_BLOCK), 0, c->stream>>>(d_p, d_cid, d_site, N, nc, d_member, vote ? d_votes : nullptr);
    HIP_TRY(c, hipGetLastError());
    if ((rc = copy_to_host(c, membership, d_member, (size_t)N * 4))) return rc;
    if (vote && (rc = copy_to_host(c, votes, d_votes, (size_t)(K * nc) * 8))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

// ---- PCA: column means, the covariance of the centred rows, the projection -------------------------------------------------------
// The order of every sum: the rows in chunks of PC_ROWS; inside a chunk one by one in ascending row, starting from 0.0; the chunk
// sums one by one in ascending chunk.  mean = sum / N; cov = sum / max(N - 1, 1).

__global__ __launch_bounds__(256) void k_pca_colsum(const double *X, i64 N, i64 D, double *partial, unsigned *status)
{
    const i64 col = (i64)blockIdx.x * 256 + threadIdx.x;
    if (col >= D) return;
    const i64 r0 = (i64)blockIdx.y * PC_ROWS, r1 = imin64(N, r0 + PC_ROWS);
    double s = 0.0;
    bool bad = false;
    for (i64 r = r0; r < r1; r++) {
        const double v = X[r * D + col];
        bad = bad || !(fabs(v) <= DP_MAX_ABS);
        s = s + v;
    }
    if (bad) atomicOr(status, 1u);
    partial[(i64)blockIdx.y * D + col] = s;
}

// out[e] = (the chunk sums of entry e, ascending) / divisor
__global__ __launch_bounds__(256) void k_pca_chunks(const double *partial, i64 n_chunks, i64 n_entries, double divisor, double *out)
{
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_entries) return;
    double s = partial[e];
    for (i64 q = 1; q < n_chunks; q++) s = s + partial[q * n_entries + e];
    out[e] = s / divisor;
}

__global__ __launch_bounds__(PC_EDGE * PC_EDGE) void k_pca_cov(const double *X, const double *mean, i64 N, i64 D, double *partial)
{
    __shared__ double A[PC_EDGE][PC_EDGE + 1], B[PC_EDGE][PC_EDGE + 1];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const i64 a0 = (i64)blockIdx.y * PC_EDGE, b0 = (i64)blockIdx.x * PC_EDGE;
    const i64 r0 = (i64)blockIdx.z * PC_ROWS, r1 = imin64(N, r0 + PC_ROWS);
    const double ma = a0 + tx < D ? mean[a0 + tx] : 0.0, mb = b0 + tx < D ? mean[b0 + tx] : 0.0;
    double acc = 0.0;
    for (i64 r = r0; r < r1; r += PC_EDGE) {
        const i64 row = r + ty;
        __syncthreads();
        A[ty][tx] = (row < r1 && a0 + tx < D) ? X[row * D + a0 + tx] - ma : 0.0;
        B[ty][tx] = (row < r1 && b0 + tx < D) ? X[row * D + b0 + tx] - mb : 0.0;
        __syncthreads();
        const int nr = (int)imin64(PC_EDGE, r1 - r);
        for (int q = 0; q < nr; q++) acc = acc + A[q][ty] * B[q][tx];
    }
    if (a0 + ty < D && b0 + tx < D) partial[(i64)blockIdx.z * D * D + (a0 + ty) * D + (b0 + tx)] = acc;
}

// Y[r, k] = sum over c ascending of (X[r, c] - mean[c]) ct[c, k]
__global__ __launch_bounds__(256) void k_pca_project(const double *X, const double *mean, const double *ct, i64 N, i64 D, int d, double *Y,
                                                     unsigned *status)
{
    const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * d) return;
    const i64 r = idx / d;
    const int k = (int)(idx - r * d);
    double s = 0.0;
    bool bad = false;
    for (i64 col = 0; col < D; col++) {
        const double v = X[r * D + col];
        bad = bad || !(fabs(v) <= DP_MAX_ABS);
        s = s + (v - mean[col]) * ct[col * d + k];
    }
    if (bad) atomicOr(status, 1u);
    Y[idx] = s;
}

static int pca_shape(sit_ctx *c, const char *who, i64 N, i64 D)
{
    char text[160];
    if (N < 1 || D < 1) {
        snprintf(text, sizeof(text), "%s: no rows or no columns", who);
        c->msg = text;
        return SIT_ERR_INVALID;
    }
    if (D > PC_MAX_D || N > PC_MAX_N) {
        snprintf(text, sizeof(text), "%s: %s", who, D > PC_MAX_D ? "more than 4096 columns" : "more than 2^25 rows");
        c->msg = text;
        return SIT_ERR_CAPACITY;
    }
    return SIT_OK;
}

static int pca_status(sit_ctx *c, const char *who, unsigned *d_status)
{
    unsigned *h_status = (unsigned *)c->h_pinned;
    HIP_TRY(c, hipMemcpyAsync(h_status, d_status, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_status[0]) {
        c->msg = std::string(who) + ": a value that is not finite or beyond 1e150";
        return SIT_ERR_INVALID;
    }
    return SIT_OK;
}

extern "C" int sit_pca_covariance(sit_ctx *c, const double *X, i64 N, i64 D, double *mean, double *cov)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    int rc = pca_shape(c, "sit_pca_covariance", N, D);
    if (rc) return rc;
    SIT_REQUIRE(c, X && mean && cov, "sit_pca_covariance: missing array");
    const i64 n_chunks = (N + PC_ROWS - 1) / PC_ROWS, DD = D * D;
    if (n_chunks * DD * 8 > PC_MAX_PARTIAL) {
        c->msg = "sit_pca_covariance: the per-chunk sums (ceil(N / 1024) D D doubles) are beyond 8 GiB";
        return SIT_ERR_CAPACITY;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    unsigned *d_status;
    double *d_mean, *d_colpart;
    rc = carve_scratch(c, [&](Carve &cv) {
        d_status = cv.take<unsigned>(16, 64); d_mean = cv.take<double>(D, 64);
    });
    if (rc) return rc;
    double *d_X, *d_part, *d_cov;
    auto lay = [&](Carve &cv) { d_X = cv.take<double>(N * D, 256); d_colpart = cv.take<double>(n_chunks * D, 256); d_part = cv.take<double>(n_chunks * DD, 256); d_cov = cv.take<double>(DD, 256); };
    Carve cv = {nullptr, 0};
    lay(cv);
    Scoped buf(c);
    HIP_TRY(c, sit_dmalloc(c, &buf.p, (size_t)cv.used));
    cv = {(char *)buf.p, 0};
    lay(cv);
    if ((rc = copy_to_device(c, d_X, X, (size_t)(N * D) * 8))) return rc;
    HIP_TRY(c, hipMemsetAsync(d_status, 0, 64, c->stream));
    k_pca_colsum<<<dim3((unsigned)((D + 255) / 256), (unsigned)n_chunks), dim3(256), 0, c->stream>>>(d_X, N, D, d_colpart, d_status);
    k_pca_chunks<<<dim3((unsigned)((D + 255) / 256)), dim3(256), 0, c->stream>>>(d_colpart, n_chunks, D, (double)N, d_mean);
    HIP_TRY(c, hipGetLastError());
    if ((rc = pca_status(c, "sit_pca_covariance", d_status))) return rc;
    const unsigned nb = (unsigned)((D + PC_EDGE - 1) / PC_EDGE);
    k_pca_cov<<<dim3(nb, nb, (unsigned)n_chunks), dim3(PC_EDGE, PC_EDGE), 0, c->stream>>>(d_X, d_mean, N, D, d_part);
    k_pca_chunks<<<dim3((unsigned)((DD + 255) / 256)), dim3(256), 0, c->stream>>>(d_part, n_chunks, DD, (double)std::max<i64>(N - 1, 1), d_cov);
    HIP_TRY(c, hipGetLastError());
    if ((rc = copy_to_host(c, mean, d_mean, (size_t)D * 8))) return rc;
    if ((rc = copy_to_host(c, cov, d_cov, (size_t)DD * 8))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

extern "C" int sit_pca_project(sit_ctx *c, const double *X, i64 N, i64 D, const double *mean, const double *comps, i64 d, double *Y)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    int rc = pca_shape(c, "sit_pca_project", N, D);
    if (rc) return rc;
    SIT_REQUIRE(c, d >= 1, "sit_pca_project: no components");
    if (d > DP_MAX_D) { c->msg = "sit_pca_project: more than 32 components (d at most 32)"; return SIT_ERR_CAPACITY; }
    SIT_REQUIRE(c, X && mean && comps && Y, "sit_pca_project: missing array");
    std::vector<double> ct((size_t)(D * d));
    for (i64 col = 0; col < D; col++) {
        SIT_REQUIRE(c, fabs(mean[col]) <= DP_MAX_ABS, "sit_pca_project: a mean that is not finite or beyond 1e150");
        for (i64 k = 0; k < d; k++) {
            const double v = comps[k * D + col];
            SIT_REQUIRE(c, fabs(v) <= DP_MAX_ABS, "sit_pca_project: a component that is not finite or beyond 1e150");
            ct[(size_t)(col * d + k)] = v;
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    unsigned *d_status;
    double *d_mean, *d_ct;
    rc = carve_scratch(c, [&](Carve &cv) {
        d_status = cv.take<unsigned>(16, 64); d_mean = cv.take<double>(D, 64); d_ct = cv.take<double>(D * d, 64);
    });
    if (rc) return rc;
    double *d_X, *d_Y;
    auto lay = [&](Carve &cv) { d_X = cv.take<double>(N * D, 256); d_Y = cv.take<double>(N * d, 256); };
    Carve cv = {nullptr, 0};
    lay(cv);
    Scoped buf(c);
    HIP_TRY(c, sit_dmalloc(c, &buf.p, (size_t)cv.used));
    cv = {(char *)buf.p, 0};
    lay(cv);
    if ((rc = copy_to_device(c, d_X, X, (size_t)(N * D) * 8))) return rc;
    if ((rc = copy_to_device(c, d_mean, mean, (size_t)D * 8))) return rc;
    if ((rc = copy_to_device(c, d_ct, ct.data(), (size_t)(D * d) * 8))) return rc;
    HIP_TRY(c, hipMemsetAsync(d_status, 0, 64, c->stream));
    k_pca_project<<<dim3((unsigned)((N * d + 255) / 256)), dim3(256), 0, c->stream>>>(d_X, d_mean, d_ct, N, D, (int)d, d_Y, d_status);
    HIP_TRY(c, hipGetLastError());
    if ((rc = pca_status(c, "sit_pca_project", d_status))) return rc;
    if ((rc = copy_to_host(c, Y, d_Y, (size_t)(N * d) * 8))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}
