// DiffusionPathwayAnalysis (network/DiffusionPathwayAnalysis.py) on the device: the image code of every connected site pair,
// the compacted edge list, and the connected components of the 3 x 3 x 3 supercell graph that the reference builds with one
// Python call per edge per image (:199-224) and hands to scipy (:76-78).  pathway_graph.h has every decision - node numbering,
// image codes, the +-1 rule, the hook and compress rules and why their fixed point is the lowest node index of each component
// whatever the order of arrival; this file has the launches.  PBCCalculator.min_image for many pairs (sit_min_image) shares
// the arithmetic.
//
// Every kernel is an ordinary finite launch: a thread handles a bounded number of entries, a label chain is followed for at
// most PG_JUMP_CAP steps, and the host decides after every round, from one word, whether another one is needed.  Labels that
// other workgroups of the same launch lower are read and written with agent-scope atomics only (a stale value is a valid,
// merely older, label: the rules are monotonic).
#include "sit_internal.h"
#include "pathway_graph.h"

#define PW_BLOCK 256

namespace {
__device__ __forceinline__ int label_load(const i32 *label, int x)
{
    return __hip_atomic_load(label + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

inline unsigned blocks_for(i64 n) { return (unsigned)((n + PW_BLOCK - 1) / PW_BLOCK); }
}

// ---- the edge pass ----------------------------------------------------------------------------------------------------------

// entry e = from * K + to of the K x K mask: code[e] = the image code of a connected pair, 0 elsewhere; *count += connected
__global__ __launch_bounds__(PW_BLOCK) void k_pw_codes(Images27 I, const unsigned char *conn, const double *centers, i64 K, i32 *code,
                                                       unsigned *count)
{
    const i64 e = (i64)blockIdx.x * PW_BLOCK + threadIdx.x;
    const bool on = e < K * K && conn[e] != 0;
    if (e < K * K) {
        int cd = 0;
        if (on) {
            const i64 from = e / K, to = e - from * K;
            const double a[3] = {centers[3 * from], centers[3 * from + 1], centers[3 * from + 2]};
            const double b[3] = {centers[3 * to], centers[3 * to + 1], centers[3 * to + 2]};
            cd = pg_pair_code(I.img, a, b);
        }
        code[e] = cd;
    }
    const unsigned long long m = __ballot(on);
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(count, (unsigned)__popcll(m));
}

// the connected entries as records (from, to, code), in whatever order the waves arrive: nothing downstream depends on it
__global__ __launch_bounds__(PW_BLOCK) void k_pw_list(const unsigned char *conn, const i32 *code, i64 K, unsigned *cursor, unsigned n_edges,
                                                      i32 *list)
{
    const i64 e = (i64)blockIdx.x * PW_BLOCK + threadIdx.x;
    const bool on = e < K * K && conn[e] != 0;
    const unsigned long long m = __ballot(on);
    if (!m) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(cursor, (unsigned)__popcll(m));
    base = __shfl(base, leader);
    if (on) {
        const unsigned at = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (at < n_edges) {                                      // (the count came from the same mask: always)
            const i64 from = e / K;
            list[3 * (i64)at] = (i32)from;
            list[3 * (i64)at + 1] = (i32)(e - from * K);
            list[3 * (i64)at + 2] = code[e];
        }
    }
}

// ---- component labelling ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(PW_BLOCK) void k_pw_init(i32 *label, i64 n_nodes)
{
    const i64 v = (i64)blockIdx.x * PW_BLOCK + threadIdx.x;
    if (v < n_nodes) label[v] = (i32)v;
}

// implicit edge t = source image * n_edges + listed edge
__global__ __launch_bounds__(PW_BLOCK) void k_pw_hook(const i32 *list, i64 n_edges, int n_images, int K, i32 *label, i64 n_nodes, unsigned *changed)
{
    const i64 t = (i64)blockIdx.x * PW_BLOCK + threadIdx.x;
    bool hooked = false;
    if (t < n_edges * n_images) {
        const int src = (int)(t / n_edges);
        const i64 e = t - (i64)src * n_edges;
        int u, v;
        if (pg_edge_nodes(n_images, K, list[3 * e], list[3 * e + 1], list[3 * e + 2], src, &u, &v)) {
            int node, value;
            hooked = pg_hook(label_load(label, u), label_load(label, v), &node, &value);
            // a label is a node of the graph; it is checked all the same before it is used as an index
            if (hooked && node >= 0 && (i64)node < n_nodes)
                __hip_atomic_fetch_min(label + node, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const unsigned long long m = __ballot(hooked);
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) __hip_atomic_store(changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(PW_BLOCK) void k_pw_compress(i32 *label, i64 n_nodes)
{
    const i64 v = (i64)blockIdx.x * PW_BLOCK + threadIdx.x;
    if (v >= n_nodes) return;
    const int own = label_load(label, (int)v);
    const int p = pg_compress([&](int x) { return (x >= 0 && (i64)x < n_nodes) ? label_load(label, x) : x; }, (int)v);
    if (p != own) __hip_atomic_store(label + v, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

extern "C" int sit_pathway_components(sit_ctx *c, i64 K, const uint8_t *conn, const double *centers, int n_images, i32 *code, i32 *root,
                                      i64 *rounds)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, K >= 0, "sit_pathway_components: negative count");
    SIT_REQUIRE(c, K <= PG_MAX_SITES, "sit_pathway_components: more than 16384 sites (the K x K mask is limited to 256 MB)");
    SIT_REQUIRE(c, n_images == 1 || n_images == 27, "sit_pathway_components: n_images is 1 (the plain site graph) or 27 (the supercell)");
    SIT_REQUIRE(c, root && rounds && (K == 0 || (conn && centers)), "sit_pathway_components: missing array");
    *rounds = 0;
    if (K == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const i64 KK = K * K, n_nodes = (i64)n_images * K;
    // scratch, every piece on a 64-byte boundary: 16 words {connected entries, list cursor, change flag, -} | labels | codes | centres | mask
    unsigned *d_words;
    i32 *d_label, *d_code;
    double *d_cen;
    unsigned char *d_conn;
    int rc = carve_scratch(c, [&](Carve &cv) {
        d_words = cv.take<unsigned>(16, 64); d_label = cv.take<i32>(n_nodes, 64); d_code = cv.take<i32>(KK, 64);
        d_cen = cv.take<double>(3 * K, 64); d_conn = cv.take<unsigned char>(KK, 64);
    });
    if (rc) return rc;
    unsigned *h_words = (unsigned *)c->h_pinned;

    if ((rc = copy_to_device(c, d_conn, conn, (size_t)KK))) return rc;
    if ((rc = copy_to_device(c, d_cen, centers, (size_t)K * 24))) return rc;
    HIP_TRY(c, hipMemsetAsync(d_words, 0, 64, c->stream));
    Images27 I;
    cp_images(c->pbc, I.img);
    k_pw_codes<<<dim3(blocks_for(KK)), dim3(PW_BLOCK), 0, c->stream>>>(I, d_conn, d_cen, K, d_code, d_words);
    k_pw_init<<<dim3(blocks_for(n_nodes)), dim3(PW_BLOCK), 0, c->stream>>>(d_label, n_nodes);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(h_words, d_words, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const i64 n_edges = (i64)h_words[0];
    if (n_edges > KK) { c->msg = "sit_pathway_components: more connected pairs counted than the mask has entries"; return SIT_ERR_CAPACITY; }

    Scoped list(c);
    i64 taken = 0;
    if (n_edges > 0) {
        HIP_TRY(c, sit_dmalloc(c, &list.p, (size_t)n_edges * 12));
        k_pw_list<<<dim3(blocks_for(KK)), dim3(PW_BLOCK), 0, c->stream>>>(d_conn, d_code, K, d_words + 1, (unsigned)n_edges, (i32 *)list.p);
        HIP_TRY(c, hipGetLastError());
        const i64 n_implicit = n_edges * n_images;
        bool settled = false;
        while (taken < n_nodes) {                                // a component of n nodes is joined after fewer rounds than that
            taken++;
            HIP_TRY(c, hipMemsetAsync(d_words + 2, 0, 4, c->stream));
            k_pw_hook<<<dim3(blocks_for(n_implicit)), dim3(PW_BLOCK), 0, c->stream>>>((const i32 *)list.p, n_edges, n_images, (int)K, d_label,
                                                                                     n_nodes, d_words + 2);
            k_pw_compress<<<dim3(blocks_for(n_nodes)), dim3(PW_BLOCK), 0, c->stream>>>(d_label, n_nodes);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(h_words, d_words + 2, 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (!h_words[0]) { settled = true; break; }
        }
        if (!settled) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            c->msg = "sit_pathway_components: the labelling did not settle within as many rounds as the graph has nodes";
            return SIT_ERR_CAPACITY;
        }
    }
    *rounds = taken;
    if (code && (rc = copy_to_host(c, code, d_code, (size_t)KK * 4))) return rc;
    if ((rc = copy_to_host(c, root, d_label, (size_t)n_nodes * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // the list goes back to the pool
    return SIT_OK;
}

// ---- PBCCalculator.min_image (util/PBCCalculator.pyx:262-316) for n pairs -------------------------------------------------

__global__ __launch_bounds__(PW_BLOCK) void k_pw_min_image(Images27 I, const double *ref, double *pts, i64 n, i32 *code)
{
    const i64 p = (i64)blockIdx.x * PW_BLOCK + threadIdx.x;
    if (p >= n) return;
    const double r[3] = {ref[3 * p], ref[3 * p + 1], ref[3 * p + 2]};
    double q[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
    code[p] = pg_min_image(I.img, r, q);
    pts[3 * p] = q[0]; pts[3 * p + 1] = q[1]; pts[3 * p + 2] = q[2];
}

extern "C" int sit_min_image(sit_ctx *c, const double *ref, double *pts, i64 n, i32 *code)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, n >= 0, "sit_min_image: negative count");
    SIT_REQUIRE(c, n == 0 || (ref && pts && code), "sit_min_image: missing array");
    SIT_REQUIRE(c, n < ((i64)1 << 31), "sit_min_image: more than 2^31 pairs");
    if (n == 0) return SIT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    double *d_ref, *d_pts;
    i32 *d_code;
    int rc = carve_scratch(c, [&](Carve &cv) { d_ref = cv.take<double>(3 * n); d_pts = cv.take<double>(3 * n); d_code = cv.take<i32>(n); });
    if (rc) return rc;
    if ((rc = copy_to_device(c, d_ref, ref, (size_t)n * 24))) return rc;
    if ((rc = copy_to_device(c, d_pts, pts, (size_t)n * 24))) return rc;
    Images27 I;
    cp_images(c->pbc, I.img);
    k_pw_min_image<<<dim3(blocks_for(n)), dim3(PW_BLOCK), 0, c->stream>>>(I, d_ref, d_pts, n, d_code);
    HIP_TRY(c, hipGetLastError());
    if ((rc = copy_to_host(c, pts, d_pts, (size_t)n * 24))) return rc;
    if ((rc = copy_to_host(c, code, d_code, (size_t)n * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIT_OK;
}
