"""ctypes binding of the van Hove entry points of ``libsitator_hip.so`` (declared in ``include/sitator_hip_vanhove.h``, the
second header of the library): a signature table of its own, set on the object ``_lib.load()`` returns, and module-level
functions that take a ``HipContext``.  ``_lib.SIGNATURES`` and the methods of ``HipContext`` stay as they are."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _d, _i, _i64, _ptr, _dp, _ip, _u64p, _vp, i64

# every symbol include/sitator_hip_vanhove.h declares: (restype, argtypes)
SIGNATURES = {
    "sit_vanhove": (C.c_int, [_vp, _dp, i64, i64, _ip, i64, _ip, i64, C.c_int, _ip, i64, i64, C.c_double, i64, C.c_int, i64, _u64p, _u64p,
                              _dp]),
    "sit_vanhove_plan": (C.c_int, [i64, i64, i64, i64, i64, i64, C.c_int, C.c_int, C.c_int, i64, _ip]),
}

PLAN_KEYS = ["threads", "max_bins", "max_atoms", "origins_per_workgroup", "b_span", "pairs_per_workgroup", "b_tiles", "window",
             "self_batch", "lds_bytes", "workspace", "self_origins_per_workgroup"]


def bind(lib):
    """Sets ``argtypes`` / ``restype`` of the two symbols on ``lib`` (once) and returns it."""
    return _lib.bind_signatures(lib, "_vanhove_bound", SIGNATURES)


def vanhove_plan(F, n_a, n_b, n_lags, n_bins, origin_stride=1, self_part=True, distinct_part=True, unwrap=True, workspace_bytes=0):
    """The plan of ``vanhove`` for these sizes (``sit_vanhove_plan``): the workgroup, the limits, the origins and atoms of ``b``
    of a distinct workgroup and its pairs, the frames per window and the atoms per batch a workspace cap allows, the LDS bytes.
    Whatever ``vanhove`` would refuse of these arguments: ``ValueError``."""
    lib = bind(_lib.load())
    rc, plan = _lib._plan(PLAN_KEYS, lambda out: lib.sit_vanhove_plan(int(F), int(n_a), int(n_b), int(n_lags), int(n_bins), int(origin_stride),
                                                                       int(bool(self_part)), int(bool(distinct_part)), int(bool(unwrap)),
                                                                       int(workspace_bytes), out))
    if rc != _lib.OK:
        raise ValueError("vanhove_plan: sizes beyond what vanhove takes, or a workspace cap below one frame or one atom")
    return plan


def vanhove(ctx, atoms_a, atoms_b, lags, r_max, n_bins, positions=None, same=False, origin_stride=1, unwrap=True, self_part=True,
            distinct_part=True, workspace_bytes=0):
    """``(self_counts, distinct_counts, max_residual)`` of ``sit_vanhove`` on the context ``ctx``: uint64
    ``[n_lags, n_bins + 1]`` each (the last entry of a row is the overflow), ``None`` for a part not asked for.  ``positions``:
    a host ``[F, A, 3]`` float64 array; without it the frames resident after ``set_frames``.  ``atoms_a`` / ``atoms_b``: columns
    of a frame; ``same``: they are one selection and the pairs of equal position in them are left out.  Reads frames only: no
    deferred pass is collected and ``labels_version`` stays.  An argument that does not fit raises ``ValueError``."""
    lib = bind(ctx.lib)
    positions, F, A = ctx._frames(positions)
    a, b = _i64(atoms_a).reshape(-1), _i64(atoms_b).reshape(-1)
    lag_arr = _i64(lags).reshape(-1)
    shape = (len(lag_arr), max(int(n_bins), 0) + 1)
    out_self = np.zeros(shape, dtype=np.uint64) if self_part else None
    out_distinct = np.zeros(shape, dtype=np.uint64) if distinct_part else None
    res = C.c_double(0.0)
    ctx._check(lib.sit_vanhove(ctx._h, _d(positions), int(F), int(A), _i(a), len(a), _i(b), len(b), int(bool(same)), _i(lag_arr), len(lag_arr),
                               int(origin_stride), float(r_max), int(n_bins), int(bool(unwrap)), int(workspace_bytes), _ptr(out_self),
                               _ptr(out_distinct), C.byref(res)))
    return out_self, out_distinct, res.value
