// The per-site point clouds of a SiteTrajectory (SiteTrajectory.real_positions_for_site, SiteTrajectory.py:160-184) for ALL
// sites at once: a stable counting sort of the assigned entries e = frame * M + ion by their label (group_plan.h has the
// plan), and on the grouped points the arithmetic of the two consumers that loop over the sites in the reference:
// misc/NAvgsPerSite.py (bucket averages with PBCCalculator.average) and site_descriptors/SiteVolumes.py:51-77 (cumulative
// recentring; the hulls of the recentred copy are hull.hip's).
//
// Order.  Sites ascending, inside a site ascending e: the order of real_traj[:, mobile_mask][traj == site].  A chunk of
// entries belongs to one wave that walks it tile by tile in ascending e, so the rank of an entry among the equal labels
// before it is (what the earlier tiles of the chunk left in the site's cursor) + (the equal labels in lower lanes of its
// tile).  The second part comes from ballots over the bits of the label, never from the order atomics land in: two ions on
// one site in one frame sit in one tile and keep their order.  The histogram may use atomics: counts have no order.
// Every label is validated by the histogram pass, whose status words the host reads before anything is indexed with one.
#include <cmath>
#include <cstdio>

#include "sit_internal.h"
#include "clamp_point.h"
#include "group_plan.h"

#define GA_BLOCK 256
#define GP_NONE 0xFFFFFFFFu

namespace {
struct GroupState {
    double *pts = nullptr, *confs = nullptr, *work = nullptr;   // [N, 3], [N], the recentred copy [N, 3]
    i64 *entries = nullptr;                                     // [N]
    i64 *d_offsets = nullptr;                                   // [K + 1]
    double *d_shift = nullptr;                                  // [K, 3] offsets of a recentring step
    std::vector<i64> offsets;                                   // [K + 1]
    i64 N = 0, K = 0, gen = -1, n_chunks = 0;
    bool valid = false;
    int lds = 1;
    i64 recenter_next = 0, recenter_n = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double ms_group = 0, ms_avg = 0, ms_recenter = 0, ms_hull = 0;
};

GroupState *state_of(sit_ctx *c)
{
    if (!c->group) c->group = new GroupState();
    return (GroupState *)c->group;
}

void drop_buffers(sit_ctx *c, GroupState *g)
{
    void *ptrs[] = {g->pts, g->confs, g->work, g->entries, g->d_offsets, g->d_shift};
    for (void *p : ptrs) if (p) sit_dfree(c, p);
    g->pts = g->confs = g->work = g->d_shift = nullptr;
    g->entries = g->d_offsets = nullptr;
    g->valid = false;
}

}

void group_free(sit_ctx *c)
{
    GroupState *g = (GroupState *)c->group;
    if (!g) return;
    drop_buffers(c, g);
    if (g->ev0) (void)hipEventDestroy(g->ev0);
    if (g->ev1) (void)hipEventDestroy(g->ev1);
    delete g;
    c->group = nullptr;
}

// ---- the counting sort ----------------------------------------------------------------------------------------------------

// status[0]: largest label >= K, + 1; status[1]: labels < -1
template <bool LDS> __global__ __launch_bounds__(GP_TILE) void k_group_hist(const i64 *labels, i64 N, i64 K, unsigned *table, u64 *status)
{
    extern __shared__ unsigned lds_row[];
    const int lane = threadIdx.x;
    const i64 chunk = blockIdx.x;
    unsigned *row = LDS ? lds_row : table + chunk * K;           // the global rows were zeroed by the host
    if (LDS) {
        for (i64 s = lane; s < K; s += GP_TILE) lds_row[s] = 0u;
        __syncthreads();
    }
    const i64 e_begin = chunk * GP_CHUNK, e_end = e_begin + GP_CHUNK < N ? e_begin + GP_CHUNK : N;
    for (i64 e = e_begin + lane; e < e_end; e += GP_TILE) {
        const i64 lab = labels[e];
        if (lab >= K) atomicMax((unsigned long long *)&status[0], (unsigned long long)lab + 1ull);
        else if (lab < -1) atomicAdd((unsigned long long *)&status[1], 1ull);
        else if (lab >= 0) atomicAdd(&row[lab], 1u);
    }
    if (LDS) {
        __syncthreads();
        for (i64 s = lane; s < K; s += GP_TILE) table[chunk * K + s] = lds_row[s];
    }
}

// per site: the counts of its chunks become the exclusive sums over the chunks; totals[site] = its entries
__global__ __launch_bounds__(256) void k_group_scan(unsigned *table, i64 n_chunks, i64 K, i64 *totals)
{
    const i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= K) return;
    unsigned run = 0;
    for (i64 c = 0; c < n_chunks; c++) {
        const unsigned v = table[c * K + s];
        table[c * K + s] = run;
        run += v;
    }
    totals[s] = (i64)run;
}

// One wave per chunk.  dest[e] = the place of entry e in the grouped arrays (GP_NONE: unassigned); the entry number and the
// confidence go there now, the position when its frame is at hand (k_group_positions).
template <bool LDS> __global__ __launch_bounds__(GP_TILE) void k_group_scatter(const i64 *labels, const double *confs, i64 N, i64 K, int bits,
                                                                              unsigned *table, const i64 *offsets, i64 n_grouped,
                                                                              unsigned *dest, double *gconfs, i64 *gentries)
{
    extern __shared__ unsigned lds_row[];
    const int lane = threadIdx.x;
    const i64 chunk = blockIdx.x;
    unsigned *row = LDS ? lds_row : table + chunk * K;
    if (LDS) {
        for (i64 s = lane; s < K; s += GP_TILE) lds_row[s] = table[chunk * K + s];
        __syncthreads();
    }
    const i64 e_begin = chunk * GP_CHUNK, e_end = e_begin + GP_CHUNK < N ? e_begin + GP_CHUNK : N;
    const u64 below = (1ull << lane) - 1ull;
    for (i64 e0 = e_begin; e0 < e_end; e0 += GP_TILE) {
        const i64 e = e0 + lane;
        const bool in = e < e_end;
        const i64 lab = in ? labels[e] : -1;
        const bool valid = lab >= 0 && lab < K;
        // the lanes of this tile with the same label: one ballot per bit of the label
        u64 peers = __ballot(valid);
        for (int b = 0; b < bits; b++) {
            const bool bit = (lab >> b) & 1;
            const u64 set = __ballot(valid && bit);
            peers &= bit ? set : ~set;
        }
        unsigned base = 0;
        if (valid) base = LDS ? row[lab] : __hip_atomic_load(&row[lab], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();                                         // every lane has read the cursor before a leader moves it
        if (valid) {
            const unsigned rank = (unsigned)__popcll(peers & below);
            if (rank == 0) {
                const unsigned next = base + (unsigned)__popcll(peers);
                if (LDS) row[lab] = next;
                else __hip_atomic_store(&row[lab], next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const i64 d = offsets[lab] + (i64)base + (i64)rank;
            if (d < n_grouped) {
                dest[e] = (unsigned)d;
                gentries[d] = e;
                gconfs[d] = confs[e];
            } else dest[e] = GP_NONE;                            // cannot happen: offsets and cursors come from the same labels
        } else if (in) dest[e] = GP_NONE;
        __syncthreads();
    }
}

// entries [e_lo, e_hi): the position of entry e = (frame f, ion m) is pos[((f - f_base) * A + midx[m]) * 3 ...]
__global__ __launch_bounds__(256) void k_group_positions(const double *pos, i64 A, const i32 *midx, i64 M, i64 e_lo, i64 e_hi, i64 f_base,
                                                         const unsigned *dest, i64 n_grouped, double *gpts)
{
    const i64 e = e_lo + (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= e_hi) return;
    const unsigned d = dest[e];
    if (d == GP_NONE || (i64)d >= n_grouped) return;
    const i64 f = e / M, m = e - f * M;
    const double *src = pos + ((f - f_base) * A + (i64)midx[m]) * 3;
    double *dst = gpts + 3 * (i64)d;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
}

extern "C" int sit_group_plan(i64 n_entries, i64 K, i64 *out4)
{
    if (!out4) return SIT_ERR_INVALID;
    const GroupPlan p = gp_plan(n_entries, K, 0);
    out4[0] = GP_CHUNK; out4[1] = p.n_chunks; out4[2] = p.lds; out4[3] = GP_LDS_MAX_SITES;
    return p.ok ? SIT_OK : SIT_ERR_CAPACITY;
}

extern "C" int sit_group_by_site(sit_ctx *c, const double *positions, i64 F, i64 A, const i64 *mobile_idx, i64 M, i64 K,
                                 i64 workspace_bytes, i64 *offsets)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid, "sit_group_by_site: assignments needed");
    SIT_REQUIRE(c, offsets, "sit_group_by_site: missing array");
    SIT_REQUIRE(c, F >= 0 && A >= 0 && M >= 0 && K >= 0 && workspace_bytes >= 0, "sit_group_by_site: negative count");
    SIT_REQUIRE(c, F == c->F, "sit_group_by_site: F is not the number of frames of the resident labels");
    SIT_REQUIRE(c, M == c->M, "sit_group_by_site: M is not the number of label columns");
    SIT_REQUIRE(c, A < ((i64)1 << 31), "sit_group_by_site: more than 2^31 atoms");
    const bool host_pos = positions != nullptr;
    std::vector<i32> m32;
    if (host_pos) {
        SIT_REQUIRE(c, mobile_idx || M == 0, "sit_group_by_site: host positions need mobile_idx");
        m32.resize((size_t)M);
        for (i64 i = 0; i < M; i++) {
            SIT_REQUIRE(c, mobile_idx[i] >= 0 && mobile_idx[i] < A, "sit_group_by_site: a mobile index outside [0, A)");
            m32[(size_t)i] = (i32)mobile_idx[i];
        }
    } else {
        SIT_REQUIRE(c, c->d_frames && c->A > 0 && c->d_mobile_idx, "sit_group_by_site: no resident frames (sit_set_frames first)");
        SIT_REQUIRE(c, A == c->A, "sit_group_by_site: A is not the number of atoms of the resident frames");
    }
    const i64 N = F * M;
    GroupPlan p = gp_plan(N, K, M);
    if (!p.ok) { c->msg = "sit_group_by_site: more than 2^31 entries, or a chunk x site table beyond 8 GB"; return SIT_ERR_CAPACITY; }
    const i64 Fs = host_pos ? gp_frames_per_stage(workspace_bytes, F, A) : F;
    SIT_REQUIRE(c, !host_pos || F == 0 || A == 0 || Fs >= 1, "sit_group_by_site: the workspace cap is below one frame");
    HIP_TRY(c, hipSetDevice(c->device));
    GroupState *g = state_of(c);
    drop_buffers(c, g);
    if (!g->ev0) { HIP_TRY(c, hipEventCreate(&g->ev0)); HIP_TRY(c, hipEventCreate(&g->ev1)); }
    g->offsets.assign((size_t)K + 1, 0);
    g->N = 0; g->K = K; g->n_chunks = p.n_chunks; g->lds = p.lds; g->recenter_next = 0; g->recenter_n = 0;

    int rc = carve_scratch(c, [&](Carve &cv) { p.lay(cv); });
    if (rc) return rc;
    const size_t lds_bytes = p.lds ? (size_t)(K > 0 ? K : 1) * 4 : 0;
    const dim3 cgrid((unsigned)(p.n_chunks > 0 ? p.n_chunks : 1));

    HIP_TRY(c, hipEventRecord(g->ev0, c->stream));
    HIP_TRY(c, hipMemsetAsync(p.status, 0, 32, c->stream));
    std::vector<i64> totals((size_t)K, 0);
    if (p.n_chunks > 0 && K > 0) {
        if (!p.lds) HIP_TRY(c, hipMemsetAsync(p.table, 0, (size_t)p.table_words * 4, c->stream));
        if (p.lds) k_group_hist<true><<<cgrid, dim3(GP_TILE), lds_bytes, c->stream>>>(c->d_labels, N, K, p.table, p.status);
        else k_group_hist<false><<<cgrid, dim3(GP_TILE), 0, c->stream>>>(c->d_labels, N, K, p.table, p.status);
        k_group_scan<<<dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream>>>(p.table, p.n_chunks, K, p.totals);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(totals.data(), p.totals, (size_t)K * 8, hipMemcpyDeviceToHost, c->stream));
    } else if (p.n_chunks > 0) {
        // no site at all: the labels are still looked at (every assigned one is beyond the sites)
        k_group_hist<true><<<cgrid, dim3(GP_TILE), lds_bytes, c->stream>>>(c->d_labels, N, K, p.table, p.status);
        HIP_TRY(c, hipGetLastError());
    }
    u64 *h_status = (u64 *)c->h_pinned;
    HIP_TRY(c, hipMemcpyAsync(h_status, p.status, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = label_status(c, "sit_group_by_site", h_status[0], h_status[1], K))) return rc;
    for (i64 s = 0; s < K; s++) g->offsets[(size_t)s + 1] = g->offsets[(size_t)s] + totals[(size_t)s];
    const i64 Ng = g->offsets[(size_t)K];
    if (Ng > N) { c->msg = "sit_group_by_site: the site counts exceed the entries"; return SIT_ERR_CAPACITY; }

    const size_t n1 = (size_t)(Ng > 0 ? Ng : 1);
    HIP_TRY(c, sit_dmalloc(c, (void **)&g->pts, n1 * 24));
    HIP_TRY(c, sit_dmalloc(c, (void **)&g->confs, n1 * 8));
    HIP_TRY(c, sit_dmalloc(c, (void **)&g->entries, n1 * 8));
    HIP_TRY(c, sit_dmalloc(c, (void **)&g->d_offsets, ((size_t)K + 1) * 8));
    HIP_TRY(c, sit_dmalloc(c, (void **)&g->d_shift, (size_t)(K > 0 ? K : 1) * 24));
    HIP_TRY(c, hipMemcpyAsync(g->d_offsets, g->offsets.data(), ((size_t)K + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(p.offsets, g->offsets.data(), ((size_t)K + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (host_pos && M > 0) HIP_TRY(c, hipMemcpyAsync(p.midx, m32.data(), (size_t)M * 4, hipMemcpyHostToDevice, c->stream));

    if (Ng > 0) {
        Scoped dest(c), stage(c);
        HIP_TRY(c, sit_dmalloc(c, &dest.p, (size_t)N * 4));
        if (p.lds) k_group_scatter<true><<<cgrid, dim3(GP_TILE), lds_bytes, c->stream>>>(
            c->d_labels, c->d_confs, N, K, p.label_bits, p.table, p.offsets, Ng, (unsigned *)dest.p, g->confs, g->entries);
        else k_group_scatter<false><<<cgrid, dim3(GP_TILE), 0, c->stream>>>(
            c->d_labels, c->d_confs, N, K, p.label_bits, p.table, p.offsets, Ng, (unsigned *)dest.p, g->confs, g->entries);
        HIP_TRY(c, hipGetLastError());
        if (!host_pos) {
            k_group_positions<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream>>>(
                c->d_frames, A, c->d_mobile_idx, M, 0, N, 0, (const unsigned *)dest.p, Ng, g->pts);
            HIP_TRY(c, hipGetLastError());
        } else {
            const i64 frame_bytes = A * 24;
            HIP_TRY(c, sit_dmalloc(c, &stage.p, (size_t)(Fs * frame_bytes)));
            for (i64 f0 = 0; f0 < F; f0 += Fs) {
                const i64 nf = f0 + Fs < F ? Fs : F - f0;
                // (copy_to_device waits for the stream first: the kernel that read the stage before is done)
                if ((rc = copy_to_device(c, stage.p, (const char *)positions + f0 * frame_bytes, (size_t)(nf * frame_bytes)))) return rc;
                const i64 e_lo = f0 * M, e_hi = (f0 + nf) * M;
                k_group_positions<<<dim3((unsigned)((e_hi - e_lo + 255) / 256)), dim3(256), 0, c->stream>>>(
                    (const double *)stage.p, A, p.midx, M, e_lo, e_hi, f0, (const unsigned *)dest.p, Ng, g->pts);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipStreamSynchronize(c->stream));
            }
        }
        HIP_TRY(c, hipEventRecord(g->ev1, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));             // dest and stage go back to the pool
    } else {
        HIP_TRY(c, hipEventRecord(g->ev1, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, g->ev0, g->ev1);
    g->ms_group = ms;
    g->N = Ng; g->gen = c->labels_gen; g->valid = true;
    for (i64 s = 0; s <= K; s++) offsets[s] = g->offsets[(size_t)s];
    return SIT_OK;
}

// the grouping of this context if it still describes the resident labels
static int current_grouping(sit_ctx *c, const char *who, GroupState **out)
{
    GroupState *g = (GroupState *)c->group;
    if (!g || !g->valid) { c->msg = std::string(who) + ": no grouping (sit_group_by_site first)"; return SIT_ERR_INVALID; }
    if (!c->assign_valid || g->gen != c->labels_gen) {
        c->msg = std::string("stale grouping: the labels were rewritten after sit_group_by_site (") + who + ")";
        return SIT_ERR_INVALID;
    }
    *out = g;
    return SIT_OK;
}

extern "C" int sit_grouped_fetch(sit_ctx *c, i64 first, i64 n, double *pts, double *confs, i64 *entries)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    GroupState *g = nullptr;
    int rc = current_grouping(c, "sit_grouped_fetch", &g);
    if (rc) return rc;
    SIT_REQUIRE(c, first >= 0 && n >= 0 && first <= g->N && n <= g->N - first, "sit_grouped_fetch: a range outside the grouping");
    if (n == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (pts && (rc = copy_to_host(c, pts, g->pts + 3 * first, (size_t)n * 24))) return rc;
    if (confs && (rc = copy_to_host(c, confs, g->confs + first, (size_t)n * 8))) return rc;
    if (entries && (rc = copy_to_host(c, entries, g->entries + first, (size_t)n * 8))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}

// ---- bucket averages: PBCCalculator.average (util/PBCCalculator.pyx:106-139) of every pts[i::n] of every site ---------

// One workgroup per bucket (site s, i): the elements of the site at ranks i, i + n, i + 2 n ...  A thread takes the elements
// t, t + 256, ... of the bucket in that order, the 256 partial results are joined by a fixed tree: the result of a bucket
// depends on its own elements only.
__global__ __launch_bounds__(GA_BLOCK) void k_group_bucket_avg(Pbc P, const double *pts, const double *confs, const i64 *offsets, i64 n_avg,
                                                               int weighted, double *out, i64 *anchors)
{
    __shared__ Best sb[GA_BLOCK];
    __shared__ double sm[4][GA_BLOCK];
    const int t = threadIdx.x;
    const i64 b = blockIdx.x, s = b / n_avg, i = b - s * n_avg;
    const i64 o = offsets[s], len = offsets[s + 1] - o;
    if (len <= n_avg) {                                          // not averaged (NAvgsPerSite.py:55,66-70)
        if (t == 0) { out[3 * b] = out[3 * b + 1] = out[3 * b + 2] = NAN; anchors[b] = -1; }
        return;
    }
    const i64 nb = (len - i + n_avg - 1) / n_avg;
    const double *bp = pts + 3 * (o + i);
    const double *bw = confs + (o + i);
    // np.argmax(weights): the first maximum (:120-122); without weights the first element
    i64 ja = 0;
    if (weighted) {
        Best best = best_empty();
        for (i64 j = t; j < nb; j += GA_BLOCK) best = best_merge(best, best_of(bw[j * n_avg], j));
        sb[t] = best;
        __syncthreads();
        for (int h = GA_BLOCK / 2; h > 0; h >>= 1) {
            if (t < h) sb[t] = best_merge(sb[t], sb[t + h]);
            __syncthreads();
        }
        ja = sb[0].i;
    }
    double off[3];
    for (int d = 0; d < 3; d++) off[d] = P.cen[d] - bp[3 * ja * n_avg + d];                        // :124
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (i64 j = t; j < nb; j += GA_BLOCK) {
        const double p[3] = {bp[3 * j * n_avg] + off[0], bp[3 * j * n_avg + 1] + off[1], bp[3 * j * n_avg + 2] + off[2]};   // :129
        double w[3], fl[3];
        cp_wrap(P, p, w, fl);                                                                      // :130
        const double wt = weighted ? bw[j * n_avg] : 1.0;
        a[0] += wt; a[1] += w[0] * wt; a[2] += w[1] * wt; a[3] += w[2] * wt;                       // :132
    }
    for (int q = 0; q < 4; q++) sm[q][t] = a[q];
    __syncthreads();
    for (int h = GA_BLOCK / 2; h > 0; h >>= 1) {
        if (t < h) for (int q = 0; q < 4; q++) sm[q][t] += sm[q][t + h];
        __syncthreads();
    }
    if (t == 0) {
        const double m[3] = {sm[1][0] / sm[0][0] - off[0], sm[2][0] / sm[0][0] - off[1], sm[3][0] / sm[0][0] - off[2]};   // :132-133
        double w[3], fl[3];
        cp_wrap(P, m, w, fl);                                                                      // :135
        out[3 * b] = w[0]; out[3 * b + 1] = w[1]; out[3 * b + 2] = w[2];
        anchors[b] = o + i + ja * n_avg;
    }
}

extern "C" int sit_grouped_bucket_averages(sit_ctx *c, i64 n_avg, int weighted, double *centers_out, i64 *anchors_out)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    GroupState *g = nullptr;
    int rc = current_grouping(c, "sit_grouped_bucket_averages", &g);
    if (rc) return rc;
    SIT_REQUIRE(c, n_avg >= 1 && centers_out, "sit_grouped_bucket_averages: n_avg >= 1 and an output array needed");
    const i64 B = g->K * n_avg;
    SIT_REQUIRE(c, B < ((i64)1 << 31), "sit_grouped_bucket_averages: more than 2^31 buckets");
    if (B == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    double *d_out;
    i64 *d_anchor;
    if ((rc = carve_scratch(c, [&](Carve &cv) { d_out = cv.take<double>(3 * B); d_anchor = cv.take<i64>(B); }))) return rc;
    HIP_TRY(c, hipEventRecord(g->ev0, c->stream));
    k_group_bucket_avg<<<dim3((unsigned)B), dim3(GA_BLOCK), 0, c->stream>>>(c->pbc, g->pts, g->confs, g->d_offsets, n_avg, weighted ? 1 : 0,
                                                                           d_out, d_anchor);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(g->ev1, c->stream));
    HIP_TRY(c, hipMemcpyAsync(centers_out, d_out, (size_t)B * 24, hipMemcpyDeviceToHost, c->stream));
    if (anchors_out) HIP_TRY(c, hipMemcpyAsync(anchors_out, d_anchor, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, g->ev0, g->ev1);
    g->ms_avg = ms;
    return SIT_OK;
}

// ---- cumulative recentring: SiteVolumes.compute_accessable_volumes (site_descriptors/SiteVolumes.py:58-62) -------------

// shift[s] = centroid - work[anchor of site s at step i]: read from the copy as the step before left it (:60)
__global__ __launch_bounds__(256) void k_group_recenter_shift(Pbc P, const double *work, const i64 *offsets, i64 K, i64 step, i64 n_steps, double *shift)
{
    const i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= K) return;
    const i64 o = offsets[s], len = offsets[s + 1] - o;
    if (len <= 0) return;                                        // the host refused such a grouping before the launch
    i64 idx = (i64)((double)step * ((double)len / (double)n_steps));
    if (idx >= len) idx = len - 1;                               // step < n_steps keeps it below len; never read past the site
    for (int d = 0; d < 3; d++) shift[3 * s + d] = P.cen[d] - work[3 * (o + idx) + d];
}

// pos += offset; wrap_points(pos) (:61-62) for every element of every site
__global__ __launch_bounds__(256) void k_group_recenter_apply(Pbc P, double *work, const i64 *offsets, i64 K, i64 N, const double *shift)
{
    const i64 d = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= N) return;
    i64 lo = 0, hi = K;                                          // the site of d: the last s with offsets[s] <= d
    while (hi - lo > 1) {
        const i64 mid = (lo + hi) >> 1;
        if (offsets[mid] <= d) lo = mid; else hi = mid;
    }
    const double p[3] = {work[3 * d] + shift[3 * lo], work[3 * d + 1] + shift[3 * lo + 1], work[3 * d + 2] + shift[3 * lo + 2]};
    double w[3], fl[3];
    cp_wrap(P, p, w, fl);
    work[3 * d] = w[0]; work[3 * d + 1] = w[1]; work[3 * d + 2] = w[2];
}

extern "C" int sit_grouped_recenter_step(sit_ctx *c, i64 i, i64 n_recenterings, double *pts_out)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    GroupState *g = nullptr;
    int rc = current_grouping(c, "sit_grouped_recenter_step", &g);
    if (rc) return rc;
    SIT_REQUIRE(c, n_recenterings >= 1 && i >= 0 && i < n_recenterings, "sit_grouped_recenter_step: step outside [0, n_recenterings)");
    SIT_REQUIRE(c, i == 0 || (i == g->recenter_next && n_recenterings == g->recenter_n),
                "sit_grouped_recenter_step: the steps come in order, from step 0, with one n_recenterings");
    for (i64 s = 0; s < g->K; s++)
        if (g->offsets[(size_t)s + 1] == g->offsets[(size_t)s]) return index_out_of_bounds(c, 0, 0);   // pos[0] of an empty site (:60)
    if (g->K == 0 || g->N == 0) { g->recenter_next = i + 1; g->recenter_n = n_recenterings; return SIT_OK; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (!g->work) HIP_TRY(c, sit_dmalloc(c, (void **)&g->work, (size_t)g->N * 24));
    if (i == 0) HIP_TRY(c, hipMemcpyAsync(g->work, g->pts, (size_t)g->N * 24, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(g->ev0, c->stream));
    k_group_recenter_shift<<<dim3((unsigned)((g->K + 255) / 256)), dim3(256), 0, c->stream>>>(c->pbc, g->work, g->d_offsets, g->K, i, n_recenterings,
                                                                                             g->d_shift);
    k_group_recenter_apply<<<dim3((unsigned)((g->N + 255) / 256)), dim3(256), 0, c->stream>>>(c->pbc, g->work, g->d_offsets, g->K, g->N, g->d_shift);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(g->ev1, c->stream));
    if (pts_out && (rc = copy_to_host(c, pts_out, g->work, (size_t)g->N * 24))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, g->ev0, g->ev1);
    g->ms_recenter = ms;
    g->recenter_next = i + 1; g->recenter_n = n_recenterings;
    return SIT_OK;
}

// hull.hip: the working copy once step 0 has been taken
int group_working_copy(sit_ctx *c, const char *who, GroupWork *out)
{
    GroupState *g = nullptr;
    int rc = current_grouping(c, who, &g);
    if (rc) return rc;
    if (g->recenter_next < 1 || (g->N > 0 && !g->work)) {
        c->msg = std::string(who) + ": no working copy (sit_grouped_recenter_step from step 0 first)";
        return SIT_ERR_INVALID;
    }
    out->work = g->work; out->d_offsets = g->d_offsets; out->N = g->N; out->K = g->K;
    out->ev0 = g->ev0; out->ev1 = g->ev1; out->ms_hull = &g->ms_hull;
    return SIT_OK;
}

extern "C" int sit_group_info(sit_ctx *c, double *out, int n)
{
    if (!c || !out) return SIT_ERR_INVALID;
    const GroupState *g = (const GroupState *)c->group;
    const double v[8] = {g ? (double)g->N : 0.0, g ? (double)g->K : 0.0, g ? (double)g->n_chunks : 0.0, g ? (double)g->lds : 0.0,
                         g ? g->ms_group : 0.0, g ? g->ms_avg : 0.0, g ? g->ms_recenter : 0.0, g ? g->ms_hull : 0.0};
    for (int k = 0; k < n; k++) out[k] = k < 8 ? v[k] : 0.0;
    return SIT_OK;
}
