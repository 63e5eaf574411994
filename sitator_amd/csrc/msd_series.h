// The unwrapped series of msd.hip as vanhove.hip shares them: the host function that runs k_msd_shift, the int32 scans and
// k_msd_series over a batch of atoms.  The cell a launch reads is that of series.h.
#pragma once
#include "series.h"
#include "msd_plan.h"

// y [nb][3][F] = x_u[t] - x_u[0] of columns [a0, a0 + nb) of the source, on c->stream.  unwrap: images [3 nb][F] and totals
// [3 nb][n_chunks] are worked in, the largest residual goes into *status (atomic maximum of the bits); else neither is touched
int msd_series_launch(sit_ctx *c, const SeriesSource &src, i64 a0, i64 nb, i64 F, const MsdCell &cell, bool unwrap, i64 n_chunks,
                      i32 *images, void *totals, double *y, u64 *status);
