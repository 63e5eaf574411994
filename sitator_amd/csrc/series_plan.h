// The plain arithmetic of the front of a frame-series call (series.h), in ONE place: the origins of a lag, the first element
// of a list outside a range, the cell a call can work with.  Host and device arithmetic only: no HIP call, no context, no side
// effect (tests/test_series_plan.py compiles it with g++ under ASan / UBSan).
#pragma once
#include <math.h>
#include <stdint.h>

#include "msd_plan.h"

// origins t = 0, s, 2 s, .. with t + tau <= F - 1 (0 <= tau <= F - 1, s >= 1)
MSD_HD int64_t series_origins(int64_t F, int64_t tau, int64_t stride) { return (F - 1 - tau) / stride + 1; }

// the first element of list outside [lo, hi], or -1
template <typename T> inline int64_t series_first_outside(const T *list, int64_t n, int64_t lo, int64_t hi)
{
    for (int64_t i = 0; i < n; i++)
        if (list[i] < lo || list[i] > hi) return i;
    return -1;
}

// cm = cell^T and its inverse: a finite determinant other than 0 and a finite inverse
inline bool series_cell_ok(const double *m, const double *ci)
{
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    bool ok = fabs(det) < INFINITY && det != 0.0;
    for (int i = 0; i < 9; i++) ok = ok && fabs(ci[i]) < INFINITY;
    return ok;
}
