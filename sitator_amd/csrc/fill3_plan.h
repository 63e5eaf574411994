// The launch shape of k_fill3, decided in ONE place: f3_plan() takes the facts of a launch (F3PlanIn) and the SITATOR_*
// knobs (F3Knobs) and returns the shape (F3Plan) - waves and frames per workgroup, survivor slots, window, task table,
// marker bytes, the slot form, the copy mode, whether the assignment is fused, and the LDS layout the kernel runs with.
// Host arithmetic only: no HIP call, no context, no side effect (tests/test_fill3_plan.py compiles it with g++).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <utility>
#include <vector>

#ifdef __HIPCC__
#define F3_HOST_DEVICE __host__ __device__
#else
#define F3_HOST_DEVICE
#endif

#define F3_EXPN 128

// LDS of a workgroup, in bytes from the start of the dynamic allocation
struct F3Layout {
    int fmax, gsync, ioninfo, etab, wave0;               // after xyz[fpb][S + M][3] at offset 0
    int o_ionrec, o_ttab, o_sv, o_nzc, o_mark, wbytes;   // inside a wave's region (prod at its offset 0)
    int total;
};
// rcap survivor slots (multiple of 8, <= 64), windows of iw ions (multiple of 4, <= 64), a task table of tt entries
// (multiple of 64), mcap marker bytes (multiple of 64, >= the candidates of a window)
F3_HOST_DEVICE inline F3Layout f3_layout(int fpb, int SM, int M, int nw, int rcap, int iw, int tt, int mcap, int fpb1)
{
    F3Layout L;
    int o = fpb * SM * 24;
    o = (o + 15) & ~15;                                  // LDS-DMA lands whole 16-byte pieces
    L.fmax = o; o += fpb * 8 + ((fpb * (SM - M) + 63) / 64) * 8;      // + a bit per static atom: LDS holds its WRAPPED position (skipw)
    L.gsync = o; o += nw * 8;                            // FUSE: arrivals per group of waves, "window spilled" per wave
    L.ioninfo = o; o += fpb * M * 8;                     // {first entry, entries | fallback bin << 8} per ion
    L.etab = o; o += F3_EXPN * 8;
    o = (o + 15) & ~15;
    L.wave0 = o;
    int w = rcap * 8;                                    // prod: the product of the terms 1 + e of every survivor
    w = (w + 15) & ~15;
    // FPB1: per NON-EMPTY list of the window, in ion order, {first entry - first task, ion} (one more than ions: an idle
    // lane may look at the entry behind the last); else per ion {first entry - first task, LDS offsets, frame} and, behind
    // them, the ion of every non-empty list
    L.o_ionrec = w; w += fpb1 ? (iw + 1) * 8 : iw * 16 + ((iw + 1 + 15) & ~15);
    L.o_ttab = w; w += tt * 4;                           // landmark << (LG + 5) | ion of the window
    L.o_sv = w; w += rcap * 4;                           // the task of every survivor
    L.o_nzc = w; w += iw * 4;                            // entries written per ion
    L.o_mark = w; w += mcap / 8 + 8;                     // a bit per candidate task of the window: set on the LAST task of every list
    L.wbytes = (w + 15) & ~15;
    L.total = L.wave0 + nw * L.wbytes;
    return L;
}

// ---- the knobs: read once per launch (tests change them between the launches of one process) ----------------------------

struct F3Knobs {
    int waves, fpb, rcap, iw, tcap;     // SITATOR_FILL_WAVES / FPB / RCAP / IW / TCAP: 0 = decided here
    int contig, wide_copy, dma;         // SITATOR_FILL_CONTIG (-1: as the index lists allow), FILL_WIDE_COPY, FILL_DMA
    int autotune;                       // SITATOR_FILL_AUTOTUNE
    int cheap, nvu, frame_mod, slot, skipwrap;      // SITATOR_F3_*
    int force_exact;                    //   tests: every pass goes round again
    int lds_pad;                        //   experiments: unused LDS per workgroup (fewer workgroups per CU)
    int prio;                           //   issue priority of phase 1 (0-3)
    int debug_stop, debug_shape;        // SITATOR_DEBUG_STOP as given (f3_debug_stop: the value a launch runs with), DEBUG_SHAPE
};

inline int f3_env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

inline F3Knobs f3_knobs_from_env()
{
    F3Knobs k;
    k.waves = f3_env_int("SITATOR_FILL_WAVES", 0); k.fpb = f3_env_int("SITATOR_FILL_FPB", 0); k.rcap = f3_env_int("SITATOR_FILL_RCAP", 0);
    k.iw = f3_env_int("SITATOR_FILL_IW", 0); k.tcap = f3_env_int("SITATOR_FILL_TCAP", 0); k.contig = f3_env_int("SITATOR_FILL_CONTIG", -1);
    k.wide_copy = f3_env_int("SITATOR_FILL_WIDE_COPY", 1); k.dma = f3_env_int("SITATOR_FILL_DMA", 1); k.autotune = f3_env_int("SITATOR_FILL_AUTOTUNE", 1);
    k.cheap = f3_env_int("SITATOR_F3_CHEAP", 1); k.force_exact = f3_env_int("SITATOR_F3_FORCE_EXACT", 0); k.nvu = f3_env_int("SITATOR_F3_NVU", 1);
    k.frame_mod = f3_env_int("SITATOR_F3_FRAME_MOD", 0); k.lds_pad = f3_env_int("SITATOR_F3_LDS_PAD", 0); k.slot = f3_env_int("SITATOR_F3_SLOT", -1);
    k.prio = f3_env_int("SITATOR_F3_PRIO", 3); k.skipwrap = f3_env_int("SITATOR_F3_SKIPWRAP", 1);
    k.debug_stop = f3_env_int("SITATOR_DEBUG_STOP", 0); k.debug_shape = f3_env_int("SITATOR_DEBUG_SHAPE", 0);
    return k;
}

// The ablation stop a launch runs with: 0 under dynamic mapping (those instantiations have no ablation build).
// (Whether the assignment may be fused is the one decision that looks at the knob as given: F3PlanIn::fuse_ok.)
inline int f3_debug_stop(const F3Knobs &k, bool dynmap) { return dynmap ? 0 : k.debug_stop; }

// ---- what the decision looks at, and what it gives ------------------------------------------------------------------------

struct F3PlanIn {
    int64_t S, M;
    int vp;                             // padded vertices per landmark: 4, 8 or 16
    int64_t W, W_tight;                 // longest candidate list of the loose and of the tight table
    bool have_tight;
    double mean_candidates, tight_mean_candidates;
    bool dynmap;                        // dynamic lattice mapping
    bool fuse_asked, fuse_ok;           // the caller wants the assignment fused; the context allows it (fill3_launch)
    bool store;
    int64_t f_lo, f_hi, F;              // the launch covers frames [f_lo, f_hi) of the F on the device
    bool idx_contig;                    // the index lists are two runs, starting at idx_s0 and idx_m0, of frames of A atoms
    int64_t idx_s0, idx_m0, A;
    bool frames_aligned16;              // the frame buffer starts on a 16-byte boundary
    bool diag, f3_ref_in_cell;          // the cheap-distance instantiations; reference positions within the cell
};

struct F3Plan {
    int nw, fpb, rcap, iw, tt, mcap;
    size_t lds;                         // dynamic LDS of a workgroup: the layout, 32 spare bytes, the pad
    bool slot;
    int slot_width;                     // the widest slots a window of this launch can take (0: the flat task space)
    int contig;                         // how a frame reaches LDS: 0 index lists, 1 two runs, 2 one run, 3 in 16-byte pieces, 4 by LDS-DMA
    bool fuse, store;
    int skipw, prio;
    bool rcap_auto, tt_auto;            // rcap / tt were left to the plan (and may be left to the autotune)
    int fpb1;                           // the one-frame-per-workgroup instantiation
    int SM, M, lds_pad;                 // what f3_plan_with needs to lay a workgroup out again
    F3Layout lay;
    const char *err;                    // null, or why there is no launch
};

// A CU has 160 KiB of LDS; a workgroup must leave 256 bytes of it alone; the frames per workgroup come down until 512 are left
#define F3_LDS_PER_CU ((size_t)160 * 1024)
#define F3_LDS_LIMIT (F3_LDS_PER_CU - 256)
#define F3_LDS_FPB_LIMIT (F3_LDS_PER_CU - 512)
// workgroups are admitted in KiB and with some slack: 5 x 31.5 KB did not run five per CU, 5 x 29.5 KB did
#define F3_LDS_ADMIT_SLACK 1535
// the register budget: seven waves per SIMD (28 per CU); eight for the sixteen-wave build (32)
#define F3_WAVES_PER_CU 28
#define F3_WAVES_PER_CU_16 32
// several frames per workgroup (four waves) only while the workgroup's LDS stays within 53 KiB
#define F3_LDS_MULTI_FRAME ((size_t)53 * 1024)

// Workgroups of `lds` bytes and nw waves a CU keeps: by LDS, capped by registers.
// Kept as found: the choice of nw also caps at max_wg = 8 (0: no cap), the task-table rule has no register cap.
inline size_t f3_wg_per_cu(size_t lds, int nw, bool reg_cap, size_t max_wg)
{
    const size_t b = (lds + F3_LDS_ADMIT_SLACK) / 1024 * 1024;
    size_t k = F3_LDS_PER_CU / b;
    if (max_wg && k > max_wg) k = max_wg;
    const size_t cap = (size_t)((nw == 16 ? F3_WAVES_PER_CU_16 : F3_WAVES_PER_CU) / nw);
    return reg_cap && k > cap ? cap : k;
}

// longest candidate list an ion can meet
inline int64_t f3_wmax(const F3PlanIn &in) { return in.have_tight ? std::max(in.W_tight, in.W) : in.W; }

// ions per wave window: the workgroup's ions dealt evenly, at least 16; at most 4096 candidate tasks
inline int f3_iw_for(const F3PlanIn &in, const F3Knobs &k, int nw, int fpb)
{
    int v;
    if (k.iw >= 1 && k.iw <= 64) v = (k.iw + 3) / 4 * 4;
    else {
        const int64_t per = ((int64_t)fpb * in.M + nw - 1) / nw;
        v = (int)(per < 16 ? 16 : (per > 64 ? 64 : (per + 3) / 4 * 4));
    }
    while (v > 4 && (int64_t)v * f3_wmax(in) > 4096) v -= 4;
    return v;
}

inline int f3_mcap_for(const F3PlanIn &in, int iw) { return (int)(((int64_t)iw * f3_wmax(in) + 63) / 64 * 64); }

inline size_t f3_lds_bytes(const F3PlanIn &in, const F3Knobs &k, int nw, int fpb, int rcap, int tt)
{
    const int iw = f3_iw_for(in, k, nw, fpb);
    return (size_t)f3_layout(fpb, (int)(in.S + in.M), (int)in.M, nw, rcap, iw, tt, f3_mcap_for(in, iw), fpb == 1 ? 1 : 0).total + 32 + (size_t)k.lds_pad;
}

// the task table should hold what a window's candidates leave behind: about half of (mean candidates per ion + 1) x
// ions, in steps of 64 up to 512
inline int f3_tt_want(const F3PlanIn &in, int iw)
{
    const double per_ion = (in.have_tight ? in.tight_mean_candidates : in.mean_candidates) + 1.0;
    const int want = (int)(0.5 * per_ion * iw) + 64;
    return want < 128 ? 128 : (want > 512 ? 512 : (want + 63) / 64 * 64);
}

// Waves per workgroup: the count that keeps the most waves on a CU (workgroups are admitted by their LDS: the frame is
// shared by a workgroup's waves) among those that leave a wave a window of >= 32 ions (or what four waves would get, if
// that is less): C2 4 waves x 7 workgroups, C3 and C4 16 x 2 (profiles/r08_plan_shapes.txt), C5 4 x 6.
// (*fpb comes down to the frames per workgroup of the four-wave shape.)
inline int f3_pick_waves(const F3PlanIn &in, const F3Knobs &k, int *fpb, int rcap, bool rcap_auto, int tt)
{
    while (*fpb > 1 && f3_lds_bytes(in, k, 4, *fpb, rcap, tt) > F3_LDS_MULTI_FRAME) (*fpb)--;
    const int f4 = *fpb;
    auto per_wave = [&](int nw) { const int64_t v = ((int64_t)(nw == 4 ? f4 : 1) * in.M + nw - 1) / nw; return v > 64 ? (int64_t)64 : v; };
    int best = 4;
    int64_t best_waves = -1;
    for (int nw : {4, 8, 16}) {
        // windows of >= 32 ions (16 for sixteen waves), or what four waves would get if that is less
        const int64_t want = std::min<int64_t>(nw == 16 ? 16 : 32, per_wave(4));
        if (per_wave(nw) < want && nw != 4) continue;
        // resident waves: whole workgroups (with fewer survivor slots if that admits one more, as f3_pick_rcap)
        int64_t waves = -1;
        for (int r : {rcap, 40, 32}) {
            if (r != rcap && !(rcap_auto && r >= 64 / in.vp && r < rcap)) continue;
            const size_t wgs = f3_wg_per_cu(f3_lds_bytes(in, k, nw, nw == 4 ? f4 : 1, r, tt), nw, true, 8);
            if (wgs == 0) continue;                                 // not one workgroup of this shape fits
            waves = std::max(waves, (int64_t)wgs * nw);
        }
        if (waves > best_waves) { best_waves = waves; best = nw; }
    }
    return best_waves < 0 ? 16 : best;                              // not even one workgroup of four or eight waves fits
}

// fewer survivor slots per wave when that admits one more workgroup per CU (a full region only costs a round)
inline int f3_pick_rcap(const F3PlanIn &in, const F3Knobs &k, int nw, int fpb, int rcap, int tt)
{
    auto wgs = [&](int r) { return f3_wg_per_cu(f3_lds_bytes(in, k, nw, fpb, r, tt), nw, true, 0); };
    for (int r : {40, 32}) if (r >= 64 / in.vp && wgs(r) > wgs(rcap)) rcap = r;
    return rcap;
}

// the largest table up to f3_tt_want that does not cost a workgroup per CU
inline int f3_pick_tt(const F3PlanIn &in, const F3Knobs &k, int nw, int fpb, int rcap)
{
    const int want = f3_tt_want(in, f3_iw_for(in, k, nw, fpb));
    auto wgs = [&](int t) { return f3_wg_per_cu(f3_lds_bytes(in, k, nw, fpb, rcap, t), nw, false, 0); };
    const size_t base = wgs(128);
    int pick = 128;
    for (int t = 192; t <= want; t += 64) if (wgs(t) == base) pick = t;
    return pick;
}

// The plan with other survivor slots and another task table (the autotune's candidates): lds and the layout follow.
// The layout is the kernel's: with more than four waves a workgroup has one frame, so fpb == 1 is its FPB1 form.
inline F3Plan f3_plan_with(F3Plan p, int rcap, int tt)
{
    p.rcap = rcap; p.tt = tt;
    p.lay = f3_layout(p.fpb, p.SM, p.M, p.nw, rcap, p.iw, tt, p.mcap, p.fpb1);
    p.lds = (size_t)p.lay.total + 32 + (size_t)p.lds_pad;
    if (!p.err && p.lds > F3_LDS_LIMIT) p.err = "sit_fill: one frame's atoms do not fit in LDS";
    return p;
}

// How a frame reaches LDS.  16-byte copies when every frame group of the launch starts on a 16-byte boundary and is an
// even number of doubles ... and by LDS-DMA (the last piece of a group may read 8 bytes past its frames: not past the
// buffer's last frame)
inline int f3_pick_contig(const F3PlanIn &in, const F3Knobs &k, int fpb)
{
    int contig = in.idx_contig ? 1 : 0;
    if (contig && in.idx_s0 == 0 && in.idx_m0 == in.S && in.A == in.S + in.M) contig = 2;
    if (k.contig >= 0 && k.contig < contig) contig = k.contig;
    const bool even_frame = ((in.S + in.M) * 3) % 2 == 0;
    const bool even_groups = fpb % 2 == 0 && in.f_lo % 2 == 0 && (in.f_hi - in.f_lo) % fpb == 0;
    if (contig == 2 && k.wide_copy && in.frames_aligned16 && (even_frame || even_groups)) contig = 3;
    if (contig == 3 && k.dma && (even_frame || even_groups || in.f_hi < in.F)) contig = 4;
    return contig;
}

// The slot form of the window (SLOT): possible with one frame per workgroup, lists of at most 64 entries in every table
// the launch can meet, no dynamic mapping and no ablation stop (the phase clocks have it).  Taken by default where it
// measured faster: four-wave workgroups whose primary table has no list longer than eight entries - every frame that
// stays on that table then runs eight slots per ion (C2: windows of 16 ions, two D0 passes in either form).
// SITATOR_F3_SLOT = 0 / 1 overrides the default where the form is possible.
inline bool f3_pick_slot(const F3PlanIn &in, const F3Knobs &k, int nw, int fpb)
{
    const int dstop = f3_debug_stop(k, in.dynmap);
    const bool possible = (nw != 4 || fpb == 1) && f3_wmax(in) <= 64 && !in.dynmap && (dstop == 0 || dstop >= 10);
    const int64_t wprim = in.have_tight ? in.W_tight : in.W;
    return possible && (k.slot < 0 ? (nw == 4 && wprim <= 8) : k.slot != 0);
}

// launch shape: nw waves share the frames of a workgroup; every wave takes windows of iw of its ions
inline F3Plan f3_plan(const F3PlanIn &in, const F3Knobs &k)
{
    F3Plan p = F3Plan();
    const int64_t M = in.M;
    p.fuse = in.fuse_asked && in.fuse_ok;
    int nw = k.waves, fpb = k.fpb, rcap = k.rcap, tt = k.tcap;
    if (fpb < 1) { int64_t f = 64 / M; if (f < 1) f = 1; if (f > 32) f = 32; fpb = (int)f; }      // about 64 ions per workgroup
    if (fpb > 32) fpb = 32;
    p.rcap_auto = rcap < 8 && !p.fuse;                         // fused: the list should hold a window's survivors (64 slots)
    if (rcap < 8) rcap = 64;
    rcap = (rcap + 7) / 8 * 8;
    if (rcap > 64) rcap = 64;
    if (rcap < 64 / in.vp) rcap = 64 / in.vp;                  // a pass of 64 / vp tasks must fit an empty region
    // entries of a wave's task table (what passed the critical-vertex test and waits for its eight lanes): 128, more
    // where the candidate lists are long (C3: 7 per ion, C5: 9)
    p.tt_auto = tt < 64 || tt > 1024;
    if (p.tt_auto) tt = 128;
    tt = (tt + 63) / 64 * 64;
    if (nw != 4 && nw != 8 && nw != 16) nw = f3_pick_waves(in, k, &fpb, rcap, p.rcap_auto, tt);
    if (nw != 4) fpb = 1;                                      // several frames per workgroup only with four waves
    if (p.rcap_auto) rcap = f3_pick_rcap(in, k, nw, fpb, rcap, tt);
    if (p.tt_auto) tt = f3_pick_tt(in, k, nw, fpb, rcap);
    while (fpb > 1 && f3_lds_bytes(in, k, nw, fpb, rcap, tt) > F3_LDS_FPB_LIMIT) fpb--;
    p.nw = nw; p.fpb = fpb; p.fpb1 = fpb == 1 ? 1 : 0;
    p.iw = f3_iw_for(in, k, nw, fpb); p.mcap = f3_mcap_for(in, p.iw);
    p.SM = (int)(in.S + M); p.M = (int)M; p.lds_pad = k.lds_pad;
    p = f3_plan_with(p, rcap, tt);
    if (!p.err && (int64_t)p.iw * f3_wmax(in) > 65536) p.err = "sit_fill: candidate lists too long for the third-generation kernel";
    p.slot = f3_pick_slot(in, k, nw, fpb);
    int width = 8;
    while (width < f3_wmax(in)) width *= 2;
    p.slot_width = p.slot ? width : 0;
    // the fused assignment sits behind the window loop (and groups the windows of 64 / iw waves): one window per wave
    if (p.fuse && (int64_t)fpb * M > (int64_t)nw * p.iw) p.fuse = false;
    p.store = in.store || !p.fuse;                             // the assignment kernels (if any) read the row buffers
    p.contig = f3_pick_contig(in, k, fpb);
    p.prio = k.prio;
    p.skipw = in.diag && !in.dynmap && in.f3_ref_in_cell && k.skipwrap ? 1 : 0;
    return p;
}

// Survivor slots and task table the autotune times, in order: the plan's own pair first; no pair twice, none beyond the
// LDS a multi-frame workgroup may take
inline std::vector<std::pair<int, int>> f3_tune_candidates(const F3Plan &p, const F3PlanIn &in)
{
    const int want = f3_tt_want(in, p.iw);
    const int min_rcap = 64 / in.vp > 32 ? 64 / in.vp : 32;
    const std::pair<int, int> cand[5] = {{p.rcap, p.tt}, {p.rcap, want}, {64, want}, {min_rcap, want}, {min_rcap, want > 256 ? 256 : want}};
    std::vector<std::pair<int, int>> out;
    for (const std::pair<int, int> &q : cand) {
        if (std::find(cand, &q, q) != &q) continue;
        if (f3_plan_with(p, q.first, q.second).lds > F3_LDS_FPB_LIMIT) continue;
        out.push_back(q);
    }
    return out;
}
