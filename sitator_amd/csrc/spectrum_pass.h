// The pass kernel of spectrum.hip as msd.hip shares it: what a launch fuses, its arguments, and the two host functions that
// launch it and keep its table of roots.
#pragma once
#include "sit_internal.h"
#include "spectrum_plan.h"

enum { SP_LOAD_PLAIN = 0, SP_LOAD_FIRST = 1, SP_LOAD_UNTWIDDLE = 2, SP_LOAD_REAL = 3 };
enum { SP_MID_FWD = 1, SP_MID_INV = 2, SP_MID_CONV = 3, SP_MID_POWER = 7 };          // bit 0: forward, bit 1: inverse
enum { SP_STORE_PLAIN = 0, SP_STORE_TWIDDLE = 1, SP_STORE_BAND = 2, SP_STORE_MSD = 3 };

struct SpArgs {
    double2 *buf;                  // [atoms of the batch][M], transformed in place
    const double *speeds;          // [atoms of the batch][n]   (SP_LOAD_REAL: any real series of length n)
    const double2 *chirp;          // [n]   w_j
    const double2 *root;           // [M]   exp(-2 pi i e / M)
    const double2 *filter;         // [M]   B, in the order the forward passes leave
    const double *freqs;           // [nbins]
    const unsigned char *fmask;    // [nbins]
    double *partial;               // [atoms of the batch][tiles][2]
    double2 *spec;                 // [atoms of the batch][nbins] or null
    const double *psum;            // SP_STORE_MSD: [series][n + 1] prefix sums of the squares
    double *msd;                   // SP_STORE_MSD: [series][nbins], nbins = lags kept
    i64 n, M, nbins, L, S, tiles;
    int bits, log_s, lines, log_lines, pad, load, mid, store;
    double inv_m;
};
// one pass of level `level` of the plan over nb lines of M points (grid.y); the table of the M-th roots that every pass
// reads, whoever asks: kept with the context until another M is asked for, so every call asks again
int sp_launch(sit_ctx *c, const SpPlan &pl, int level, SpArgs a, int load, int mid, int store, i64 nb);
int sp_roots(sit_ctx *c, i64 M, const double2 **root);
