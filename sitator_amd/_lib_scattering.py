"""ctypes binding of the scattering entry points of ``libsitator_hip.so`` (declared in ``include/sitator_hip_scattering.h``, the
third header of the library): a signature table of its own, set on the object ``_lib.load()`` returns, and module-level functions
that take a ``HipContext``.  ``_lib.SIGNATURES``, ``_lib_vanhove.SIGNATURES`` and the methods of ``HipContext`` stay as they are."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import _d, _i, _i64, _ptr, _triple, _dp, _ip, _vp, i64

# every symbol include/sitator_hip_scattering.h declares: (restype, argtypes)
SIGNATURES = {
    "sit_scattering": (C.c_int, [_vp, _dp, i64, i64, _ip, i64, _ip, i64, C.c_int, _ip, i64, _ip, i64, i64, i64, _dp, _dp]),
    "sit_scattering_plan": (C.c_int, [i64, i64, i64, C.c_int, i64, _ip, i64, i64, C.c_int, C.c_int, i64, _ip]),
}

PLAN_KEYS = ["threads", "max_index", "origins_per_block", "tile_entries", "lds_bytes", "n_blocks", "q_batch", "n_q_batches", "window",
             "lags_per_launch", "workspace", "lags_per_workgroup"]


def bind(lib):
    """Sets ``argtypes`` / ``restype`` of the two symbols on ``lib`` (once) and returns it."""
    return _lib.bind_signatures(lib, "_scattering_bound", SIGNATURES)


def _q_list(q_int):
    q = _i64(q_int)
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError("q_int is a list of integer triples (h, k, l)")
    return q


def scattering_plan(F, n_a, n_b, n_q, h_max, n_lags, origin_stride=1, same=False, self_part=True, coherent_part=True, workspace_bytes=0):
    """The plan of ``scattering`` for these sizes (``sit_scattering_plan``): the workgroup, the limits, the origins of a block, the
    entries of a tile of power tables and the LDS bytes, the blocks, and the q vectors per batch, the frames per window and the
    lags per launch a workspace cap allows.  ``h_max``: the largest ``|index|`` of every axis of the q list.  Whatever
    ``scattering`` would refuse of these arguments: ``ValueError``."""
    lib = bind(_lib.load())
    H = _triple(h_max, "h_max")
    rc, plan = _lib._plan(PLAN_KEYS, lambda out: lib.sit_scattering_plan(int(F), int(n_a), int(n_b), int(bool(same)), int(n_q), _i(H), int(n_lags),
                                                                          int(origin_stride), int(bool(self_part)), int(bool(coherent_part)),
                                                                          int(workspace_bytes), out))
    if rc != _lib.OK:
        raise ValueError("scattering_plan: sizes beyond what scattering takes, or a workspace cap below one q vector and one frame")
    return plan


def scattering(ctx, atoms_a, atoms_b, q_int, lags, positions=None, same=False, origin_stride=1, self_part=True, coherent_part=True,
               workspace_bytes=0):
    """``(self_sums, coherent_sums)`` of ``sit_scattering`` on the context ``ctx``: complex128 ``[n_lags, n_q]`` each, the raw
    sums over the origins (and, for the self part, the atoms); ``None`` for a part not asked for.  ``positions``: a host
    ``[F, A, 3]`` float64 array; without it the frames resident after ``set_frames``.  ``atoms_a`` / ``atoms_b``: columns of a
    frame; ``same``: they are one selection.  ``q_int``: ``[n_q, 3]`` integer triples.  Reads frames only: no deferred pass is
    collected and ``labels_version`` stays.  An argument that does not fit raises ``ValueError``."""
    lib = bind(ctx.lib)
    positions, F, A = ctx._frames(positions)
    a, b = _i64(atoms_a).reshape(-1), _i64(atoms_b).reshape(-1)
    q, lag_arr = _q_list(q_int), _i64(lags).reshape(-1)
    shape = (len(lag_arr), len(q))
    out_self = np.zeros(shape, dtype=np.complex128) if self_part else None
    out_coherent = np.zeros(shape, dtype=np.complex128) if coherent_part else None
    ctx._check(lib.sit_scattering(ctx._h, _d(positions), int(F), int(A), _i(a), len(a), _i(b), len(b), int(bool(same)), _i(q), len(q),
                                  _i(lag_arr), len(lag_arr), int(origin_stride), int(workspace_bytes), _ptr(out_self), _ptr(out_coherent)))
    return out_self, out_coherent
