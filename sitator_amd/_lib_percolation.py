"""ctypes binding of the percolation entry points of ``libsitator_hip.so`` (declared in ``include/sitator_hip_percolation.h``, the
fifth header of the library): a signature table of its own, set on the object ``_lib.load()`` returns, and module-level functions
that take a ``HipContext``.  The four other tables and the methods of ``HipContext`` stay as they are."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _d, _i, _grid3, _ptr, _triple, _dp, _ip, _i32p, _vp, i64

# every symbol include/sitator_hip_percolation.h declares: (restype, argtypes)
SIGNATURES = {
    "sit_percolation_components": (C.c_int, [_vp, _dp, _ip, C.c_double, C.c_int, C.c_int, _i32p, i64, _ip, C.POINTER(i64), _ip]),
    "sit_percolation_levels": (C.c_int, [_vp, _dp, _ip, C.c_int, C.c_int, _dp, _i32p, _ip]),
    "sit_percolation_plan": (C.c_int, [_ip, C.c_int, C.c_int, _ip]),
}

PLAN_KEYS = ["threads", "tile0", "tile1", "tile2", "lds_bytes", "tiles", "form", "seam_records_max", "workspace", "voxels", "blocks",
             "record_words"]
RECORD_WORDS = 12                                                   # root, size, rank, basis[9]


def bind(lib):
    """Sets ``argtypes`` / ``restype`` of the three symbols on ``lib`` (once) and returns it."""
    return _lib.bind_signatures(lib, "_percolation_bound", SIGNATURES)


def percolation_plan(grid, connectivity=26, form=0):
    """The plan of the two calls for a grid ``(n0, n1, n2)`` (``sit_percolation_plan``): the workgroup, the tile of the local phase and
    its LDS bytes, the form that 0 resolves to, the seam records of the full grid and the bytes of the work area.  Whatever the
    calls would refuse of these arguments: ``ValueError``."""
    lib = bind(_lib.load())
    g = _triple(grid, "grid")
    rc, plan = _lib._plan(PLAN_KEYS, lambda out: lib.sit_percolation_plan(_i(g), int(connectivity), int(form), out))
    if rc != _lib.OK:
        raise ValueError("percolation_plan: an axis outside [1, 1024], more than 2^27 voxels, a connectivity other than 6, 18, 26 or a "
                         "form outside {0, 1, 2}")
    return plan


def percolation_components(ctx, grid, level, connectivity=26, form=0, want_labels=True):
    """``(labels, records, info)`` of ``sit_percolation_components`` on the context ``ctx``: ``labels`` int32 of the grid's shape
    (``None`` with ``want_labels=False``), ``records`` int64 ``[n, 12]`` - root, size, rank and the nine entries of the basis of
    every component in ascending root - and ``info`` = (rounds, seam records, form taken, distinct seam records)."""
    lib = bind(ctx.lib)
    grid, g = _grid3(grid)
    labels = np.empty(grid.shape, dtype=np.int32) if want_labels else None
    info = np.zeros(4, dtype=np.int64)
    rec = ctx._records(RECORD_WORDS, lambda cap, out, n: lib.sit_percolation_components(
        ctx._h, _d(grid), _i(g), float(level), int(connectivity), int(form), _ptr(labels), cap, out, n, _i(info)))
    return labels, np.ascontiguousarray(rec), tuple(int(v) for v in info)


def percolation_levels(ctx, grid, connectivity=26, form=0):
    """``(levels float64 [3], ranks int32 [3], info)`` of ``sit_percolation_levels``: ``info`` = (labelling passes, rounds of the
    last pass, seam records of the last pass, form taken)."""
    lib = bind(ctx.lib)
    grid, g = _grid3(grid)
    levels = np.zeros(3, dtype=np.float64)
    ranks = np.zeros(3, dtype=np.int32)
    info = np.zeros(4, dtype=np.int64)
    ctx._check(lib.sit_percolation_levels(ctx._h, _d(grid), _i(g), int(connectivity), int(form), _d(levels), _ptr(ranks), _i(info)))
    return levels, ranks, tuple(int(v) for v in info)
