// EnergyLandscape on the device: the energy of one probe ion at the centre of every voxel of a periodic grid, in the frozen lattice
// of the static atoms under the truncated and shifted 12-6 potential of barrier_plan.h (no counterpart in the reference; DESIGN.md
// section 25).  landscape_plan.h has every decision - the voxel centre, the term, the order of the sum, the tile and its list, the
// chunks, the limits; this file has the launches.
//
//   k_landscape_atoms    the staged form of the static atoms (bp_atom)
//   k_landscape_direct   form 1: a workgroup per tile of voxels, a thread per voxel; the atoms pass through LDS in tiles of BP_TILE
//                        records, every lane reads the same record (a broadcast) and walks that atom's translations at its own voxel
//   k_landscape_tiled    form 2: the workgroup lists the (s, m) that can lie within rc of its tile, LP_BLOCK atoms at a time - a
//                        thread counts the triples of its atom, a prefix sum over the workgroup gives them their places, the records
//                        go to LDS in list order - and every thread runs each chunk of LP_CHUNK records for its own voxel
// Every thread adds its voxel's terms in ascending (s, m0, m1, m2), alone: the same bytes in both forms and on every call.  The
// counters of info4 are integer atomics.  Float64 throughout; plain loads and stores.
#include "sit_internal.h"
#include "landscape_plan.h"
#include "sitator_hip_landscape.h"

__global__ __launch_bounds__(LP_BLOCK) void k_landscape_atoms(Pbc pbc, const double *pos, const double *eps, const double *sigma, double rc, i64 S,
                                                              double *rec)
{
    const i64 s = (i64)blockIdx.x * LP_BLOCK + threadIdx.x;
    if (s >= S) return;
    const double p[3] = {pos[3 * s], pos[3 * s + 1], pos[3 * s + 2]};
    double r[BP_REC];
    bp_atom(pbc, p, eps[s], sigma[s], rc, r);
    for (int k = 0; k < BP_REC; k++) rec[s * BP_REC + k] = r[k];
}

namespace {
// this thread's voxel of the tile: its flat index (-1 outside a partial tile), its crystal coordinates and its centre
__device__ __forceinline__ i64 lp_my_voxel(const Pbc &pbc, const LandscapePlan &p, const LpTile &tl, double f[3], double x[3])
{
    i64 i[3];
    const bool live = lp_tile_voxel(tl, (int)threadIdx.x, i);
    for (int a = 0; a < 3; a++) f[a] = lp_frac(i[a], p.n[a]);
    lp_center(pbc, f, x);
    return live ? (i[0] * p.n[1] + i[1]) * p.n[2] + i[2] : -1;
}

// a wave's sum of `mine` onto words[0], one atomic per wave
__device__ __forceinline__ void lp_count(u64 mine, u64 *words)
{
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(words, mine);
}
}

// grid: the tiles.  words[0] += the triples walked
template <class Phi>
__global__ __launch_bounds__(LP_BLOCK) void k_landscape_direct(Pbc pbc, LandscapePlan p, const double *rec, i64 S, double *energies, u64 *words)
{
    __shared__ double tile[BP_TILE * BP_REC];
    const LpTile tl = lp_tile(p, (i64)blockIdx.x);
    double f[3], x[3];
    const i64 v = lp_my_voxel(pbc, p, tl, f, x);
    double e = 0.0;
    u64 walked = 0;
    for (i64 first = 0; first < S; first += BP_TILE) {
        const int count = (int)(S - first < BP_TILE ? S - first : BP_TILE);
        if (first) __syncthreads();                              // every wave is done with the tile before
        for (int k = threadIdx.x; k < count * BP_REC; k += LP_BLOCK) tile[k] = rec[first * BP_REC + k];
        __syncthreads();
        if (v >= 0)
            for (int a = 0; a < count; a++) walked += (u64)lp_atom_add<Phi>(pbc, p.bp, tile + a * BP_REC, x, f, e);
    }
    if (v >= 0) energies[v] = e;
    lp_count(walked, words);
}

// grid: the tiles.  words[0] += the entries of the tile's list, words[1] = max(its chunks)
template <class Phi>
__global__ __launch_bounds__(LP_BLOCK) void k_landscape_tiled(Pbc pbc, LandscapePlan p, const double *rec, i64 S, double *energies, u64 *words)
{
    __shared__ double list[LP_CHUNK * LP_REC];
    __shared__ i64 wave_sum[LP_BLOCK / 64];
    const LpTile tl = lp_tile(p, (i64)blockIdx.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double f[3], x[3];
    const i64 v = lp_my_voxel(pbc, p, tl, f, x);
    double e = 0.0;
    int fill = 0;                                                // the same in every thread, like everything that steers the loops
    i64 chunks = 0, entries = 0;
    for (i64 first = 0; first < S; first += LP_BLOCK) {
        const i64 s = first + threadIdx.x;
        int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        double atom[BP_REC] = {0.0};
        i64 cnt = 0;
        if (s < S) {
            for (int k = 0; k < BP_REC; k++) atom[k] = rec[s * BP_REC + k];
            cnt = lp_tile_range(p.bp, tl, atom + 3, lo, hi);
        }
        i64 incl = cnt;                                          // the places of this thread's entries in the batch
        for (int d = 1; d < 64; d <<= 1) {
            const i64 up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        __syncthreads();                                         // the wave sums of the batch before are read
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        i64 off = incl - cnt, total = 0;
        for (int w = 0; w < LP_BLOCK / 64; w++) {
            if (w < wave) off += wave_sum[w];
            total += wave_sum[w];
        }
        for (i64 done = 0; done < total;) {
            const i64 room = LP_CHUNK - fill, take = total - done < room ? total - done : room;
            i64 k0, k1;
            lp_window(off, cnt, done, done + take, &k0, &k1);
            for (i64 k = k0; k < k1; k++) lp_record(pbc, atom, lo, hi, k, list + (fill + (off + k - done)) * LP_REC);
            fill += (int)take; done += take;
            if (fill == LP_CHUNK) {
                __syncthreads();
                if (v >= 0) lp_run_chunk<Phi>(list, fill, x, p.bp.rc2, e);
                __syncthreads();                                 // every thread is done with the chunk before it is written again
                chunks++;
                fill = 0;
            }
        }
        entries += total;
    }
    if (fill) {
        __syncthreads();
        if (v >= 0) lp_run_chunk<Phi>(list, fill, x, p.bp.rc2, e);
        chunks++;
    }
    if (v >= 0) energies[v] = e;
    if (threadIdx.x == 0) {
        if (entries) atomicAdd(words, (u64)entries);
        atomicMax(words + 1, (u64)chunks);
    }
}

namespace {
struct CellOnly { double cm[9]; };                               // what lp_plan reads of a cell
}

extern "C" int sit_landscape_plan(const double *cell, double rc, const i64 *grid3, int form, i64 *out16)
{
    if (!cell || !grid3 || !out16) return SIT_ERR_INVALID;
    CellOnly c;
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) c.cm[3 * k + j] = cell[3 * j + k];
    const LandscapePlan p = lp_plan(c, rc, grid3, form);
    const bool ok = !p.err;
    const i64 out[LP_PLAN_WORDS] = {LP_TILE0, LP_TILE1, LP_TILE2, LP_BLOCK, p.form == LP_FORM_TILED ? LP_LDS_TILED : LP_LDS_DIRECT, LP_CHUNK,
                                    p.n_tiles, p.form, ok ? p.bp.n[0] : 0, ok ? p.bp.n[1] : 0, ok ? p.bp.n[2] : 0, p.wide[0], p.wide[1],
                                    p.wide[2], p.V, BP_TILE};
    for (int i = 0; i < LP_PLAN_WORDS; i++) out16[i] = out[i];
    return ok ? SIT_OK : SIT_ERR_INVALID;
}

extern "C" int sit_landscape_energies(sit_ctx *c, const double *static_pos, const double *eps, const double *sigma, i64 S, double rc,
                                      const i64 *grid3, int form, double *energies, i64 *info4)
{
    if (!c) return SIT_ERR_INVALID;
    SIT_REQUIRE(c, static_pos && eps && sigma && grid3 && energies && info4, "sit_landscape_energies: missing array");
    SIT_REQUIRE(c, S >= 1, "sit_landscape_energies: no static atom");
    SIT_REQUIRE(c, S < ((i64)1 << 31), "sit_landscape_energies: more than 2^31 atoms");
    SIT_REQUIRE(c, rc > 0.0 && rc < INFINITY, "sit_landscape_energies: rc is not positive");
    const LandscapePlan p = lp_plan(c->pbc, rc, grid3, form);
    if (p.err) { c->msg = std::string("sit_landscape_energies: ") + p.err; return SIT_ERR_INVALID; }
    for (i64 s = 0; s < S; s++) {
        SIT_REQUIRE(c, eps[s] > 0.0 && eps[s] < INFINITY && sigma[s] > 0.0 && sigma[s] < INFINITY,
                    "sit_landscape_energies: a non-positive epsilon or sigma");
        double f[3];
        cp_to_cell(c->pbc, static_pos + 3 * s, f);
        SIT_REQUIRE(c, fabs(f[0]) <= BP_MAX_FRAC && fabs(f[1]) <= BP_MAX_FRAC && fabs(f[2]) <= BP_MAX_FRAC,
                    "sit_landscape_energies: a static atom that is not finite or more than 2^20 cells from the origin");
    }
    HIP_TRY(c, hipSetDevice(c->device));

    // a pool buffer of the call, every piece on a 256-byte boundary: records | raw positions | eps | sigma | energies | counters
    double *d_rec, *d_pos, *d_eps, *d_sig, *d_en;
    u64 *d_words;
    Scoped work(c);
    int rc_ = carve_scratch(c, [&](Carve &cv) {
        d_rec = cv.take<double>(S * BP_REC, 256); d_pos = cv.take<double>(3 * S, 256); d_eps = cv.take<double>(S, 256);
        d_sig = cv.take<double>(S, 256); d_en = cv.take<double>(p.V, 256); d_words = cv.take<u64>(2, 256);
    }, &work);
    if (rc_) return rc_;
    if ((rc_ = copy_to_device(c, d_pos, static_pos, (size_t)S * 24))) return rc_;
    if ((rc_ = copy_to_device(c, d_eps, eps, (size_t)S * 8))) return rc_;
    if ((rc_ = copy_to_device(c, d_sig, sigma, (size_t)S * 8))) return rc_;
    HIP_TRY(c, hipMemsetAsync(d_words, 0, 16, c->stream));
    k_landscape_atoms<<<dim3((unsigned)((S + LP_BLOCK - 1) / LP_BLOCK)), dim3(LP_BLOCK), 0, c->stream>>>(c->pbc, d_pos, d_eps, d_sig, rc, S, d_rec);
    if (p.form == LP_FORM_TILED)
        k_landscape_tiled<LpLJ><<<dim3((unsigned)p.n_tiles), dim3(LP_BLOCK), 0, c->stream>>>(c->pbc, p, d_rec, S, d_en, d_words);
    else
        k_landscape_direct<LpLJ><<<dim3((unsigned)p.n_tiles), dim3(LP_BLOCK), 0, c->stream>>>(c->pbc, p, d_rec, S, d_en, d_words);
    HIP_TRY(c, hipGetLastError());
    u64 *h_words = (u64 *)c->h_pinned;
    HIP_TRY(c, hipMemcpyAsync(h_words, d_words, 16, hipMemcpyDeviceToHost, c->stream));
    if ((rc_ = copy_to_host(c, energies, d_en, (size_t)p.V * 8))) return rc_;
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // the buffer goes back to the pool
    info4[0] = p.form; info4[1] = p.n_tiles; info4[2] = (i64)h_words[1]; info4[3] = (i64)h_words[0];
    return SIT_OK;
}
