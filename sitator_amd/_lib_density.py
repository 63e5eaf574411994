"""ctypes binding of the density entry points of ``libsitator_hip.so`` (declared in ``include/sitator_hip_density.h``, the fourth
header of the library): a signature table of its own, set on the object ``_lib.load()`` returns, and module-level functions that
take a ``HipContext``.  The three other tables and the methods of ``HipContext`` stay as they are."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _d, _i, _i32, _i64, _f64, _grid3, _ptr, _triple, _dp, _ip, _i32p, _u64p, _vp, i64

# every symbol include/sitator_hip_density.h declares: (restype, argtypes)
SIGNATURES = {
    "sit_density": (C.c_int, [_vp, _dp, i64, i64, _ip, i64, i64, _ip, _i32p, i64, i64, _ip, _dp, i64, C.c_int, i64, _u64p, _dp, _ip]),
    "sit_density_peaks": (C.c_int, [_vp, _dp, _ip, C.c_double, i64, _ip, C.POINTER(i64)]),
    "sit_density_plan": (C.c_int, [i64, i64, i64, i64, _ip, i64, i64, i64, _ip, C.c_int, C.c_int, i64, _ip]),
}

PLAN_KEYS = ["threads", "table_slots", "probe_limit", "lds_bytes", "frames_per_run", "runs", "form", "tile0", "tile1", "tile2",
             "ext0", "ext1", "ext2", "smooth_lds_bytes", "window", "n_windows", "workspace", "frames_taken", "voxels", "cells"]


def bind(lib):
    """Sets ``argtypes`` / ``restype`` of the three symbols on ``lib`` (once) and returns it."""
    return _lib.bind_signatures(lib, "_density_bound", SIGNATURES)


def density_plan(F, A, n_sel, grid, frame_stride=1, K=0, n_classes=1, n_taps=0, halo=(0, 0, 0), form=0, host=True, workspace_bytes=0):
    """The plan of ``density`` for these sizes (``sit_density_plan``): the workgroup, the slots and the probe limit of the LDS table,
    the frames of a run and the runs, the form that 0 resolves to, the smoothing tile and the tile with its halo, and the frames
    per upload window and the work area a workspace cap allows.  ``halo``: the largest ``|d_a|`` of the taps.  Whatever ``density``
    would refuse of these arguments: ``ValueError``."""
    lib = bind(_lib.load())
    g, h = _triple(grid, "grid"), _triple(halo, "halo")
    rc, plan = _lib._plan(PLAN_KEYS, lambda out: lib.sit_density_plan(int(F), int(A), int(n_sel), int(frame_stride), _i(g), int(K), int(n_classes),
                                                                       int(n_taps), _i(h), int(form), int(bool(host)), int(workspace_bytes), out))
    if rc != _lib.OK:
        raise ValueError("density_plan: sizes beyond what density takes, or a workspace cap below one run of frames")
    return plan


def density(ctx, atoms, grid, positions=None, frame_stride=1, site_class=None, n_classes=1, taps=None, weights=None, form=0,
            workspace_bytes=0):
    """``(counts, smoothed, frames taken, skipped)`` of ``sit_density`` on the context ``ctx``: ``counts`` uint64
    ``[n_classes, n0, n1, n2]``, ``smoothed`` float64 of that shape or ``None`` without taps.  ``positions``: a host ``[F, A, 3]``
    float64 array; without it the frames resident after ``set_frames``.  ``atoms``: columns of a frame.  ``site_class``: int32
    ``[K]``, the class of every site - the entries are then split by the resident labels (a deferred pass is collected first), and
    the selection must be the label columns; without it the call reads frames only and ``labels_version`` stays.  A label beyond
    ``site_class`` raises ``IndexError``, any other argument that does not fit ``ValueError``."""
    lib = bind(ctx.lib)
    positions, F, A = ctx._frames(positions)
    a, g = _i64(atoms).reshape(-1), _triple(grid, "grid")
    sc = None
    if site_class is not None:
        sc = _i32(site_class).reshape(-1)
        if ctx._deferred:                                          # the labels are read: as HipContext's own label readers
            rc, _, err = ctx.fill_result()
            ctx._check(rc, err)
    t = w = None
    if taps is not None:
        t, w = _i64(taps), _f64(weights).reshape(-1)
        if t.ndim != 2 or t.shape[1] != 3 or len(t) != len(w):
            raise ValueError("taps is a list of integer triples with one weight each")
    n_classes = int(n_classes)
    shape = (max(n_classes, 0),) + tuple(max(int(v), 0) for v in g)
    if n_classes > 16 or any(v > 1024 for v in g) or int(np.prod(shape, dtype=np.int64)) > 1 << 27:    # before the outputs are made
        raise ValueError("sit_density: an axis of the grid holds 1 to 1024 voxels, 1 to 16 classes are needed, and 2^27 voxels at most")
    counts = np.zeros(shape, dtype=np.uint64)
    smoothed = np.zeros(shape, dtype=np.float64) if t is not None and len(t) else None
    info = np.zeros(2, dtype=np.int64)
    rc = lib.sit_density(ctx._h, _d(positions), int(F), int(A), _i(a), len(a), int(frame_stride), _i(g), _ptr(sc), 0 if sc is None else len(sc),
                         n_classes, _i(t), _d(w), 0 if t is None else len(t), int(form), int(workspace_bytes), _ptr(counts), _d(smoothed),
                         _i(info))
    ctx._check_index(rc)
    return counts, smoothed, int(info[0]), int(info[1])


def density_peaks(ctx, grid, threshold):
    """The voxels (int64, ascending) of the 3-D float64 array ``grid`` that pass the peak rule of ``sit_density_peaks``."""
    lib = bind(ctx.lib)
    grid, g = _grid3(grid)
    rec = ctx._records(1, lambda cap, out, n: lib.sit_density_peaks(ctx._h, _d(grid), _i(g), float(threshold), cap, out, n))
    return np.ascontiguousarray(rec[:, 0])
