// GenerateClampedTrajectory (misc/GenerateClampedTrajectory.pyx:92-126): for every frame and atom the atom's real position,
// its fixed position in the structure, or the centre of the site the resident labels name for it - with wrap = False the
// periodic image of that centre nearest the atom's real position (clamp_point.h).
//
// One kernel, one pass.  The output of a chunk of frames is ONE contiguous run of doubles, and so are the positions it
// is made from: a workgroup takes 256 consecutive (frame, atom) elements - 768 doubles, 6 KB - reads the positions that
// are needed into an LDS tile with consecutive lanes on consecutive addresses (16 bytes per lane where the run starts on
// a 16-byte boundary), lets lane t turn element t of the tile into its output in place, and writes the tile out the way
// it was read.  A lane per atom straight on global memory would have every load and store instruction touch 24-byte
// strides.  The per-site tables (centre, wrapped centre, crystal centre: 72 bytes a site, made once per call by
// k_clamp_sites) are gathered by label through the caches; labels are read once, by the lane that needs them.
// A label is looked at before anything is indexed with it: the smallest unassigned (frame, column), the largest label
// beyond the sites and the number of labels below -1 go to three status words that come back with every chunk.
#include <cstdio>
#include <cstdlib>

#include "sit_internal.h"
#include "clamp_point.h"

#define CL_TILE 256
#define CL_DEFAULT_WORKSPACE ((i64)1 << 30)

enum { CL_NEED_NEVER = 0, CL_NEED_ALWAYS = 1, CL_NEED_UNASSIGNED = 2 };

struct ClampArgs {
    Pbc pbc;
    Images27 img;
    const double *pos;            // [frames of the chunk][A][3] or null when no position is needed
    double *out;                   // [frames of the chunk][A][3]
    const i64 *labels;             // [F][M] from the chunk's first frame
    const i32 *role;               // [A]
    const unsigned char *need;     // [A]
    const double *fixed;           // [A][3]
    const ClampSite *sites;        // [K]
    u64 *status;                   // [0] smallest unassigned frame * M + column, [1] largest label >= K, + 1, [2] labels < -1
    i64 E, A, M, K, f0;            // E: elements (frame, atom) of the chunk; f0: its first frame
    int wrap, pass;
};

__global__ __launch_bounds__(256) void k_clamp_sites(Pbc P, const double *centers, i64 K, ClampSite *sites)
{
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const double cen[3] = {centers[3 * k], centers[3 * k + 1], centers[3 * k + 2]};
    sites[k] = cp_site(P, cen);
}

// atom of the element `o` places after one whose atom is a_start (o < 2 CL_TILE, A < 2^31 - 2 CL_TILE)
__device__ __forceinline__ unsigned cl_atom(unsigned a_start, unsigned o, unsigned A) { return (a_start + o) % A; }

template <bool VEC2> __global__ __launch_bounds__(CL_TILE) void k_clamp(ClampArgs a)
{
    __shared__ __align__(16) double tile[3 * CL_TILE];
    const int t = threadIdx.x;
    const i64 e0 = (i64)blockIdx.x * CL_TILE;
    const int n = (int)(a.E - e0 < CL_TILE ? a.E - e0 : CL_TILE), nd = 3 * n;
    const i64 f_start = e0 / a.A;
    const unsigned A = (unsigned)a.A, a_start = (unsigned)(e0 - f_start * a.A);
    const double *src = a.pos ? a.pos + 3 * e0 : nullptr;
    double *dst = a.out + 3 * e0;

    if (src) {
        if (VEC2) {
            for (int q = t; q < nd / 2; q += CL_TILE) {
                const unsigned el0 = (unsigned)(2 * q) / 3u, el1 = (unsigned)(2 * q + 1) / 3u;
                if (a.need[cl_atom(a_start, el0, A)] == CL_NEED_ALWAYS || a.need[cl_atom(a_start, el1, A)] == CL_NEED_ALWAYS)
                    ((double2 *)tile)[q] = ((const double2 *)src)[q];
            }
            if ((nd & 1) && t == 0 && a.need[cl_atom(a_start, (unsigned)(n - 1), A)] == CL_NEED_ALWAYS) tile[nd - 1] = src[nd - 1];
        } else {
            for (int i = t; i < nd; i += CL_TILE)
                if (a.need[cl_atom(a_start, (unsigned)i / 3u, A)] == CL_NEED_ALWAYS) tile[i] = src[i];
        }
    }
    __syncthreads();

    if (t < n) {
        const unsigned at = a_start + (unsigned)t, wraps = at / A;
        const i64 atom = at - wraps * A, f = a.f0 + f_start + wraps;
        const i32 role = a.role[atom];
        double o[3] = {0.0, 0.0, 0.0};
        bool keep = false;                                       // the tile already holds the real position
        if (role == -1) keep = true;
        else if (role == -2) { o[0] = a.fixed[3 * atom]; o[1] = a.fixed[3 * atom + 1]; o[2] = a.fixed[3 * atom + 2]; }
        else {
            const i64 lab = a.labels[(f - a.f0) * a.M + role];
            if (lab == -1) {
                if (!a.pass) atomicMin((unsigned long long *)&a.status[0], (unsigned long long)(f * a.M + role));
                else if (a.wrap) { o[0] = src[3 * t]; o[1] = src[3 * t + 1]; o[2] = src[3 * t + 2]; }
                else keep = true;
            }
            else if (lab >= a.K) atomicMax((unsigned long long *)&a.status[1], (unsigned long long)lab + 1ull);
            else if (lab < -1) atomicAdd((unsigned long long *)&a.status[2], 1ull);
            else if (a.wrap) { const double *cen = a.sites[lab].center; o[0] = cen[0]; o[1] = cen[1]; o[2] = cen[2]; }
            else {
                const double p[3] = {tile[3 * t], tile[3 * t + 1], tile[3 * t + 2]};
                cp_clamp_point(a.pbc, a.img.img, a.sites[lab], p, o);
            }
        }
        if (!keep) { tile[3 * t] = o[0]; tile[3 * t + 1] = o[1]; tile[3 * t + 2] = o[2]; }
    }
    __syncthreads();

    if (VEC2) {
        for (int q = t; q < nd / 2; q += CL_TILE) ((double2 *)dst)[q] = ((const double2 *)tile)[q];
        if ((nd & 1) && t == 0) dst[nd - 1] = tile[nd - 1];
    } else {
        for (int i = t; i < nd; i += CL_TILE) dst[i] = tile[i];
    }
}

static i64 clamp_default_workspace()
{
    const char *e = getenv("SITATOR_CLAMP_WORKSPACE_MB");
    const long long mb = e && *e ? atoll(e) : 0;
    return mb > 0 ? (i64)mb << 20 : CL_DEFAULT_WORKSPACE;
}

extern "C" int sit_clamp_trajectory(sit_ctx *c, const double *positions, i64 F, i64 A, const i32 *role, const double *fixed_pos,
                                    const double *centers, i64 K, int wrap, int pass_through_unassigned, i64 workspace_bytes,
                                    double *out, i64 *first_unassigned)
{
    if (!c) return SIT_ERR_INVALID;
    if (first_unassigned) *first_unassigned = -1;
    SIT_SETTLE(c);
    SIT_REQUIRE(c, c->assign_valid, "sit_clamp_trajectory: assignments needed");
    SIT_REQUIRE(c, F >= 0 && A >= 0 && K >= 0 && workspace_bytes >= 0, "sit_clamp_trajectory: negative count");
    SIT_REQUIRE(c, A < ((i64)1 << 31) - 2 * CL_TILE, "sit_clamp_trajectory: more than 2^31 atoms");
    SIT_REQUIRE(c, F == c->F, "sit_clamp_trajectory: F is not the number of frames of the resident labels");
    const i64 M = c->M;
    if (F == 0 || A == 0) return SIT_OK;
    SIT_REQUIRE(c, role && fixed_pos && out && (K == 0 || centers), "sit_clamp_trajectory: missing array");
    std::vector<unsigned char> need((size_t)A), taken((size_t)M, 0);
    bool any_need = false;
    for (i64 i = 0; i < A; i++) {
        const i32 r = role[i];
        SIT_REQUIRE(c, r >= -2 && r < M, "sit_clamp_trajectory: a role outside [-2, M)");
        if (r >= 0) {
            SIT_REQUIRE(c, !taken[(size_t)r], "sit_clamp_trajectory: two atoms with the same label column");
            taken[(size_t)r] = 1;
        }
        need[(size_t)i] = r == -1 ? CL_NEED_ALWAYS : r == -2 ? CL_NEED_NEVER : !wrap ? CL_NEED_ALWAYS
                          : pass_through_unassigned ? CL_NEED_UNASSIGNED : CL_NEED_NEVER;
        any_need = any_need || need[(size_t)i] != CL_NEED_NEVER;
    }
    const bool host_pos = any_need && positions != nullptr;
    if (any_need && !positions) {
        SIT_REQUIRE(c, c->d_frames && c->A > 0, "sit_clamp_trajectory: no resident frames (sit_set_frames first)");
        SIT_REQUIRE(c, A == c->A, "sit_clamp_trajectory: A is not the number of atoms of the resident frames");
    }
    // frames per chunk: the output, on the host path the staged positions next to it.  Chunks start on 16-byte boundaries
    // where they can (an even number of frames when a frame is an odd number of doubles).
    const i64 cap = workspace_bytes > 0 ? workspace_bytes : clamp_default_workspace();
    const i64 frame_bytes = A * 24, per_frame = frame_bytes * (host_pos ? 2 : 1);
    i64 Fc = cap / per_frame;
    SIT_REQUIRE(c, Fc >= 1, "sit_clamp_trajectory: the workspace cap is below one frame");
    if (Fc > F) Fc = F;
    if (Fc > 1 && Fc < F && (A & 1)) Fc &= ~(i64)1;
    const bool vec2 = (Fc == F || ((Fc * A * 3) & 1) == 0) && (host_pos || !any_need || ((size_t)c->d_frames & 15) == 0);
    HIP_TRY(c, hipSetDevice(c->device));

    // small tables in the scratch buffer
    u64 *d_status;
    ClampSite *d_sites;
    double *d_cen, *d_fixed;
    i32 *d_role;
    unsigned char *d_need;
    int rc = carve_scratch(c, [&](Carve &cv) {
        d_status = cv.take<u64>(3); d_sites = cv.take<ClampSite>(K); d_cen = cv.take<double>(3 * K); d_fixed = cv.take<double>(3 * A);
        d_role = cv.take<i32>(A); d_need = cv.take<unsigned char>(A);
    });
    if (rc) return rc;
    u64 *h_status = (u64 *)c->h_pinned;
    h_status[0] = ~0ull; h_status[1] = 0; h_status[2] = 0;
    HIP_TRY(c, hipMemcpyAsync(d_status, h_status, 24, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_fixed, fixed_pos, (size_t)A * 24, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_role, role, (size_t)A * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_need, need.data(), (size_t)A, hipMemcpyHostToDevice, c->stream));
    if (K > 0) {
        HIP_TRY(c, hipMemcpyAsync(d_cen, centers, (size_t)K * 24, hipMemcpyHostToDevice, c->stream));
        k_clamp_sites<<<dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream>>>(c->pbc, d_cen, K, d_sites);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // h_status is reused for the read-backs

    Scoped buf_out(c), buf_pos(c);
    HIP_TRY(c, sit_dmalloc(c, &buf_out.p, (size_t)(Fc * frame_bytes)));
    if (host_pos) HIP_TRY(c, sit_dmalloc(c, &buf_pos.p, (size_t)(Fc * frame_bytes)));
    ClampArgs a;
    a.pbc = c->pbc;
    cp_images(c->pbc, a.img.img);
    a.out = (double *)buf_out.p; a.role = d_role; a.need = d_need; a.fixed = d_fixed; a.sites = d_sites; a.status = d_status;
    a.A = A; a.M = M; a.K = K; a.wrap = wrap ? 1 : 0; a.pass = pass_through_unassigned ? 1 : 0;
    for (i64 f0 = 0; f0 < F; f0 += Fc) {
        const i64 nf = f0 + Fc < F ? Fc : F - f0;
        const size_t bytes = (size_t)(nf * frame_bytes);
        if (host_pos) {
            if ((rc = copy_to_device(c, buf_pos.p, (const char *)positions + f0 * frame_bytes, bytes))) return rc;
            a.pos = (const double *)buf_pos.p;
        } else {
            a.pos = any_need ? c->d_frames + f0 * A * 3 : nullptr;
        }
        a.labels = c->d_labels + f0 * M; a.E = nf * A; a.f0 = f0;
        const dim3 grid((unsigned)((a.E + CL_TILE - 1) / CL_TILE));
        StageTimer t(c, T_CLAMP);                               // the kernel alone: slot 7 of sit_timers
        if (vec2) k_clamp<true><<<grid, dim3(CL_TILE), 0, c->stream>>>(a);
        else k_clamp<false><<<grid, dim3(CL_TILE), 0, c->stream>>>(a);
        t.stop();
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h_status, d_status, 24, hipMemcpyDeviceToHost, c->stream));
        if ((rc = copy_to_host(c, (char *)out + f0 * frame_bytes, buf_out.p, bytes))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if ((rc = label_status(c, "sit_clamp_trajectory", h_status[1], h_status[2], K))) return rc;
        if (h_status[0] != ~0ull) {
            // an ion to clamp is unassigned and nothing passes it through: the smallest index of this chunk is the
            // smallest of all (chunks are taken in frame order)
            if (first_unassigned) *first_unassigned = (i64)h_status[0];
            char text[160];
            snprintf(text, sizeof(text), "sit_clamp_trajectory: label column %lld is unassigned at frame %lld",
                     (long long)(h_status[0] % (u64)M), (long long)(h_status[0] / (u64)M));
            c->msg = text;
            return SIT_ERR_UNASSIGNED;
        }
    }
    return SIT_OK;
}
