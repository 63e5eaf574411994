"""ctypes binding of ``libsitator_hip.so`` (C-ABI declared in ``include/sitator_hip.h``).

There is no CPU fallback: if the library is missing, or a call fails, this module raises.
"""
import ctypes as C
import functools
import os

import numpy as np

from . import errors

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SITATOR_LIB") or os.path.join(_HERE, "lib", "libsitator_hip.so")     # SITATOR_LIB: another build (A/B runs)

OK, E_INVALID, E_HIP, E_STATIC_THRESHOLD, E_STATIC_UNASSIGNED, E_ZERO_LANDMARK, \
    E_MULTIPLE_OCCUPANCY, E_NOT_CONVERGED, E_CAPACITY, RETRY, E_UNASSIGNED = range(11)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)
_vp = C.c_void_p
i64 = C.c_int64

# the pointer type an array's dtype names (complex128: the library sees pairs of doubles)
_POINTER_OF = {np.dtype(np.float64): _dp, np.dtype(np.complex128): _dp, np.dtype(np.int64): _ip, np.dtype(np.int32): _i32p,
               np.dtype(np.uint8): _u8p, np.dtype(np.uint64): _u64p}


def _ptr(a, T=None):
    """The address of the array ``a`` as the pointer type its dtype names (``T``: as that type instead); ``None`` stays
    ``None``.  The library is never handed the address of an array that is not C-contiguous or of another dtype."""
    if a is None:
        return None
    assert a.flags.c_contiguous, "the library reads C-contiguous arrays"
    T = T or _POINTER_OF.get(a.dtype)
    if T is None:
        raise TypeError("no pointer type for an array of %s" % a.dtype)
    return a.ctypes.data_as(T)


def _d(a):
    assert a is None or a.dtype == np.float64
    return _ptr(a)


def _i(a):
    assert a is None or a.dtype == np.int64
    return _ptr(a)


def _void(a):
    return _ptr(a, _vp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _opt(convert, a):
    """``convert(a)`` of an optional array, ``None`` of none."""
    return None if a is None else convert(a)


class SitError(C.Structure):
    _fields_ = [("kind", C.c_int32), ("frame", C.c_int64), ("index", C.c_int64), ("aux", C.c_int64)]


class FillParams(C.Structure):
    """``sit_fill_params``; ``struct_size`` is filled in by ``make`` (the library refuses any other size)."""
    _fields_ = [("struct_size", C.c_uint32), ("dynamic_lattice_mapping", C.c_int32), ("relaxed_lattice_checks", C.c_int32),
                ("check_for_zeros", C.c_int32), ("store_rows", C.c_int32), ("assign", C.c_int32),
                ("predict_normed", C.c_int32), ("defer", C.c_int32), ("predict_threshold", C.c_double)]

    @classmethod
    def make(cls, dynamic_lattice_mapping=0, relaxed_lattice_checks=0, check_for_zeros=1, store_rows=1, assign=0,
             predict_normed=1, predict_threshold=0.0, defer=0):
        return cls(C.sizeof(cls), int(dynamic_lattice_mapping), int(relaxed_lattice_checks), int(check_for_zeros),
                   int(store_rows), int(assign), int(predict_normed), int(defer), float(predict_threshold))


ABI_VERSION = 14       # SIT_ABI_VERSION of include/sitator_hip.h this table was written against


# every symbol include/sitator_hip.h declares: (restype, argtypes)
SIGNATURES = {
    "sit_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "sit_create": (C.c_int, [_dp, _dp, C.c_int, C.POINTER(_vp)]),
    "sit_destroy": (None, [_vp]),
    "sit_release_cached_memory": (None, []),
    "sit_last_message": (C.c_char_p, [_vp]),
    "sit_abi": (C.c_int, [_i32p, C.c_int]),
    "sit_wrap_points": (C.c_int, [_vp, _dp, i64]),
    "sit_distances": (C.c_int, [_vp, _dp, _dp, i64, _dp]),
    "sit_average": (C.c_int, [_vp, _dp, _dp, i64, _dp]),
    "sit_min_image": (C.c_int, [_vp, _dp, _dp, i64, _i32p]),
    "sit_site_vertex_distances": (C.c_int, [_vp, _dp, _dp, _ip, i64, i64, i64, _dp]),
    "sit_set_basis": (C.c_int, [_vp, _dp, i64, _ip, _dp, i64, i64, C.c_double, C.c_double, C.c_double]),
    "sit_set_frames": (C.c_int, [_vp, _dp, i64, i64, _ip, i64, _ip, i64, i64]),
    "sit_set_frames_device": (C.c_int, [_vp, _vp, i64, i64, _ip, i64, _ip, i64, i64]),
    "sit_frames_device_ptr": (C.c_int, [_vp, C.POINTER(_vp)]),
    "sit_fill": (C.c_int, [_vp, C.POINTER(FillParams), _ip, C.POINTER(SitError)]),
    "sit_fill_result": (C.c_int, [_vp, _ip, C.POINTER(SitError)]),
    "sit_upload_fill_fit": (C.c_int, [_vp, _dp, i64, i64, _ip, i64, _ip, i64, i64, C.POINTER(FillParams), C.c_double, _ip,
                                      C.POINTER(SitError), C.POINTER(C.c_int)]),
    "sit_static_seen": (C.c_int, [_vp, i64, _u8p]),
    "sit_row_width": (C.c_int, [_vp, _ip]),
    "sit_get_rows_dense": (C.c_int, [_vp, i64, i64, _dp]),
    "sit_get_rows_sparse": (C.c_int, [_vp, i64, i64, _i32p, _i32p, _dp]),
    "sit_set_rows_dense": (C.c_int, [_vp, _dp, i64, i64]),
    "sit_fit_reset": (C.c_int, [_vp]),
    "sit_fit_set_state": (C.c_int, [_vp, _dp, _ip, i64]),
    "sit_fit_get_state": (C.c_int, [_vp, _dp, _ip, _ip]),
    "sit_fit_push_stored_rows": (C.c_int, [_vp, C.c_double]),
    "sit_fit_push_dense_rows": (C.c_int, [_vp, _dp, _ip, i64, C.c_double]),
    "sit_set_centers": (C.c_int, [_vp, _dp, i64, C.c_int]),
    "sit_predict": (C.c_int, [_vp, C.c_double, _ip, _dp, _ip]),
    "sit_get_assignments": (C.c_int, [_vp, _ip, _dp, _ip]),
    "sit_count_zero_rows": (C.c_int, [_vp, _ip, _ip]),
    "sit_gram": (C.c_int, [_vp, _dp, _ip]),
    "sit_gram_limbs": (C.c_int, [_vp, _u64p, _u64p, _ip]),
    "sit_weighted_row_sums_limbs": (C.c_int, [_vp, C.c_int, i64, _u64p, _u64p]),
    "sit_best_match": (C.c_int, [_vp, _dp, _ip, _dp, _dp]),
    "sit_best_match_groups": (C.c_int, [_vp, _i32p, _dp, i64, _ip, _dp, _dp]),
    "sit_weighted_row_sums": (C.c_int, [_vp, C.c_int, i64, _dp, _dp]),
    "sit_site_anchors": (C.c_int, [_vp, C.c_int, i64, _dp, _ip, _dp]),
    "sit_site_sums": (C.c_int, [_vp, C.c_int, i64, _dp, _dp]),
    "sit_check_occupancy": (C.c_int, [_vp, i64, i64, _ip, _ip, _ip, C.POINTER(SitError)]),
    "sit_set_assignments": (C.c_int, [_vp, _ip, _dp, i64, i64, i64]),
    "sit_site_counts": (C.c_int, [_vp, i64, _ip]),
    "sit_cooccupancy": (C.c_int, [_vp, i64, _u8p]),
    "sit_jump_sources": (C.c_int, [_vp, C.c_int, _ip, _ip, _ip]),
    "sit_jump_list": (C.c_int, [_vp, C.c_int, _ip, i64, _ip, _ip, _ip]),
    "sit_jump_analysis": (C.c_int, [_vp, i64, _ip, _ip, _dp, _dp, _ip, _ip, _ip, _ip, _ip]),
    "sit_assign_last_known": (C.c_int, [_vp, i64, _ip, _ip, _ip, _i32p, _ip, _ip, _ip]),
    "sit_label_ends": (C.c_int, [_vp, _ip, _ip]),
    "sit_replace_unassigned": (C.c_int, [_vp, C.c_int, _ip, _ip, _ip]),
    "sit_unknown_runs": (C.c_int, [_vp, _ip, _ip, i64, _ip, _ip, _ip]),
    "sit_replace_closer": (C.c_int, [_vp, _ip, i64, _dp, i64, _dp, i64, _ip]),
    "sit_running_mode": (C.c_int, [_vp, i64, i64, i64, C.c_int, _ip, i64, _ip]),
    "sit_recenter_resident": (C.c_int, [_vp, _dp, _dp, _dp]),
    "sit_recenter": (C.c_int, [_vp, _dp, i64, i64, _dp, _dp, _dp]),
    "sit_speed_spectrum": (C.c_int, [_vp, _dp, i64, _ip, i64, _dp, _u8p, i64, _dp, _dp, _dp, _dp]),
    "sit_msd": (C.c_int, [_vp, _dp, i64, _ip, i64, C.c_int, i64, _ip, i64, C.c_int, i64, _dp, _dp, _dp, _i32p, _dp]),
    "sit_clamp_trajectory": (C.c_int, [_vp, _dp, i64, i64, _i32p, _dp, _dp, i64, C.c_int, C.c_int, i64, _dp, _ip]),
    "sit_group_by_site": (C.c_int, [_vp, _dp, i64, i64, _ip, i64, i64, i64, _ip]),
    "sit_grouped_fetch": (C.c_int, [_vp, i64, i64, _dp, _dp, _ip]),
    "sit_grouped_bucket_averages": (C.c_int, [_vp, i64, C.c_int, _dp, _ip]),
    "sit_grouped_recenter_step": (C.c_int, [_vp, i64, i64, _dp]),
    "sit_group_plan": (C.c_int, [i64, i64, _ip]),
    "sit_group_info": (C.c_int, [_vp, _dp, C.c_int]),
    "sit_grouped_hull_volumes": (C.c_int, [_vp, _dp, _i32p, _i32p, _u8p]),
    "sit_grouped_work_fetch": (C.c_int, [_vp, i64, i64, _dp]),
    "sit_hull_plan": (C.c_int, [_ip]),
    "sit_pathway_components": (C.c_int, [_vp, i64, _u8p, _dp, C.c_int, _i32p, _i32p, _ip]),
    "sit_barrier_energies": (C.c_int, [_vp, _dp, _dp, _dp, i64, C.c_double, _dp, i64, _i32p, i64, _dp, i64, C.c_double, _dp, _u8p,
                                       _i32p]),
    "sit_barrier_plan": (C.c_int, [_dp, C.c_double, _ip]),
    "sit_voronoi_nodes": (C.c_int, [_vp, _dp, i64, C.c_double, i64, i64, _ip, _ip, _dp, _dp, _ip, _i32p, _i32p, _i32p, _dp]),
    "sit_voronoi_plan": (C.c_int, [_dp, i64, _ip, _dp]),
    "sit_coordination_environments": (C.c_int, [_vp, _dp, i64, _dp, i64, C.c_double, C.c_double, C.c_double, C.c_double, i64, _ip, _i32p,
                                                _i32p, _i32p, _ip, _i32p, _dp, _dp, _i32p, _dp, _dp, _dp, _dp]),
    "sit_coordenv_plan": (C.c_int, [_ip, _i32p, _dp]),
    "sit_soap_vectors": (C.c_int, [_vp, _dp, _i32p, i64, _dp, i64, C.c_double, C.c_double, C.c_double, i64, i64, i64, C.c_int, _dp, _dp,
                                   i64, _dp, _i32p]),
    "sit_soap_plan": (C.c_int, [_dp, C.c_double, i64, i64, i64, _ip]),
    "sit_soap_site_averages": (C.c_int, [_vp, _dp, i64, i64, _ip, _i32p, i64, _ip, i64, i64, i64, i64, i64, C.c_double, C.c_double,
                                         C.c_double, i64, i64, i64, C.c_int, _dp, _dp, i64, i64, i64, _ip, _ip, _ip, _dp, _dp]),
    "sit_dpc_plan": (C.c_int, [i64, _ip]),
    "sit_pca_covariance": (C.c_int, [_vp, _dp, i64, i64, _dp, _dp]),
    "sit_pca_project": (C.c_int, [_vp, _dp, i64, i64, _dp, _dp, i64, _dp]),
    "sit_dpc_graph": (C.c_int, [_vp, _dp, i64, i64, C.c_double, _dp, _dp, _dp, _i32p, _dp]),
    "sit_dpc_assign": (C.c_int, [_vp, _dp, _dp, _i32p, i64, C.c_double, C.c_double, _ip, i64, _i32p, _i32p, _ip, _ip, i64]),
    "sit_comm_unique_id": (C.c_int, [_u8p]),
    "sit_comm_create": (C.c_int, [_vp, _u8p, C.c_int, C.c_int]),
    "sit_comm_destroy": (C.c_int, [_vp]),
    "sit_comm_info": (C.c_int, [_vp, _i32p]),
    "sit_comm_allreduce": (C.c_int, [_vp, _vp, i64, C.c_int, C.c_int]),
    "sit_comm_allgather": (C.c_int, [_vp, _vp, _vp, i64]),
    "sit_comm_broadcast": (C.c_int, [_vp, _vp, i64, C.c_int]),
    "sit_comm_barrier": (C.c_int, [_vp]),
    "sit_comm_attach": (C.c_int, [_vp, _vp]),
    "sit_timers": (C.c_int, [_vp, _dp, C.c_int]),
    "sit_info": (C.c_int, [_vp, _dp, C.c_int]),
    "sit_candidate_table": (C.c_int, [_vp, C.c_int, _i32p, _dp, _dp, _ip, i64, _i32p, i64, _i32p, _u8p]),
    "sit_synchronize": (C.c_int, [_vp]),
}

_lib = None


def load():
    """Load the shared library (no GPU needed for loading); raises if it was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: build it with `make -C sitator_amd/csrc` (or __graft_entry__.build()). "
                "sitator_amd has no CPU fallback." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        # the struct declarations above against the library's own layout (sit_abi): a stale binding fails at import
        abi = (C.c_int32 * 6)()
        lib.sit_abi(abi, 6)
        mine = (ABI_VERSION, C.sizeof(SitError), C.sizeof(FillParams), FillParams.predict_threshold.offset,
                SitError.frame.offset, 128)
        if tuple(abi) != mine:
            raise ImportError("%s was built from another include/sitator_hip.h: its layout %r, this binding's %r "
                              "(rebuild with `make -C sitator_amd/csrc`)" % (LIB_PATH, tuple(abi), mine))
        _lib = lib
    return _lib


def bind_signatures(lib, flag, signatures):
    """Sets ``argtypes`` / ``restype`` of every symbol of a further header's table on ``lib`` (once: ``flag`` is the attribute
    that remembers it) and returns ``lib``."""
    if not getattr(lib, flag, False):
        for name, (res, args) in signatures.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        setattr(lib, flag, True)
    return lib


def _triple(v, what):
    v = _i64(v).reshape(-1)
    if len(v) != 3:
        raise ValueError("%s holds one number per axis" % what)
    return v


def _grid3(grid):
    """``(grid as float64, its shape as int64)`` of a 3-D array."""
    grid = _f64(grid)
    if grid.ndim != 3:
        raise ValueError("grid is a 3-D array")
    return grid, _i64(grid.shape)


def comm_unique_id():
    """ncclGetUniqueId: 128 bytes that rank 0 makes and every rank of the job receives."""
    uid = np.zeros(128, dtype=np.uint8)
    if load().sit_comm_unique_id(_ptr(uid)) != 0:
        raise RuntimeError("sit_comm_unique_id failed (librccl.so not loadable?)")
    return uid.tobytes()


def device_count():
    n = C.c_int(0)
    load().sit_device_count(C.byref(n))
    return n.value


def _plan(keys, call):
    """``(status, {key: word})`` of a plan entry point that writes ``len(keys)`` int64 words through ``call(out_ptr)``."""
    out = np.zeros(len(keys), dtype=np.int64)
    rc = call(_i(out))
    return rc, {k: int(v) for k, v in zip(keys, out)}


def _translations(plan):
    return plan.pop("n0"), plan.pop("n1"), plan.pop("n2")


def group_plan(n_entries, K):
    """``(entries per chunk, chunks, LDS form, largest K of the LDS form)`` of ``group_by_site`` (``sit_group_plan``)."""
    rc, plan = _plan(["per_chunk", "chunks", "lds", "lds_max_k"], lambda out: load().sit_group_plan(int(n_entries), int(K), out))
    if rc != OK:
        raise ValueError("group_plan: beyond the capacity of group_by_site")
    return plan["per_chunk"], plan["chunks"], bool(plan["lds"]), plan["lds_max_k"]


def hull_plan():
    """``(facet capacity, open-edge capacity, threads per workgroup, LDS bytes per workgroup)`` of ``grouped_hull_volumes``
    (``sit_hull_plan``)."""
    return tuple(_plan(["facets", "edges", "threads", "lds_bytes"], lambda out: load().sit_hull_plan(out))[1].values())


def barrier_plan(cell, rc):
    """``{"translations": (n0, n1, n2), "tile": static atoms per LDS tile, "threads": per workgroup, "lds_bytes": per workgroup}``
    of ``barrier_energies`` for ``cell`` (rows are the cell vectors) and the cutoff ``rc`` (``sit_barrier_plan``)."""
    cell = _f64(cell).reshape(3, 3)
    status, plan = _plan(["n0", "n1", "n2", "tile", "threads", "lds_bytes"],
                         lambda out: load().sit_barrier_plan(_d(cell), float(rc), out))
    if status != OK:
        raise ValueError("barrier_plan: a degenerate cell, or rc not positive or beyond 255 perpendicular heights of the cell")
    plan["translations"] = _translations(plan)
    return plan


def soap_plan(cell, cutoff, n_species, n_max, l_max):
    """The plan of ``soap_vectors`` / ``soap_site_averages`` for ``cell`` (rows are the cell vectors) (``sit_soap_plan``): the
    translations, the workgroup, the neighbours staged at once, the LDS bytes, the limits and the lengths of a vector.  Beyond a
    limit: ``RuntimeError``."""
    cell = _f64(cell).reshape(3, 3)
    keys = ["n0", "n1", "n2", "threads", "nbr_cap", "lds_bytes", "max_l", "max_n", "max_species", "n_coef", "n_dim", "n_dim_crossover"]
    rc, plan = _plan(keys, lambda out: load().sit_soap_plan(_d(cell), float(cutoff), int(n_species), int(n_max), int(l_max), out))
    if rc == E_CAPACITY:
        raise RuntimeError("soap_plan: l_max, n_max or the number of environment species is beyond %r"
                           % {k: plan[k] for k in ("max_l", "max_n", "max_species")})
    if rc != OK:
        raise ValueError("soap_plan: a degenerate cell, or a cutoff not positive or beyond 255 perpendicular heights of the cell")
    plan["translations"] = _translations(plan)
    return plan


def dpc_plan(d=1):
    """The plan of ``dpc_graph`` for points of ``d`` coordinates (``sit_dpc_plan``): the workgroup, the tile, the digits and passes
    of the radix select, the limits and the LDS bytes.  Beyond the largest ``d``: ``RuntimeError``."""
    keys = ["threads", "tile", "digit_bits", "passes", "max_d", "lds_bytes", "segments", "max_n", "pca_rows", "pca_edge", "pca_max_d",
            "pca_max_n"]
    rc, plan = _plan(keys, lambda out: load().sit_dpc_plan(int(d), out))
    if rc == E_CAPACITY:
        raise RuntimeError("dpc_plan: more than %d coordinates per point" % plan["max_d"])
    if rc != OK:
        raise ValueError("dpc_plan: d must be at least 1")
    return plan


def voronoi_plan(cell, S):
    """The plan of ``voronoi_nodes`` for ``cell`` (rows are the cell vectors) and ``S`` atoms (``sit_voronoi_plan``): the caps, the
    workgroup, and the first search radius with its growth factor."""
    rad = np.zeros(2)
    cell = _f64(cell).reshape(3, 3)
    keys = ["neighbour_cap", "record_cap", "member_cap", "threads", "lds_bytes", "max_rounds", "record_bytes", "inverse_shape_min"]
    rc, plan = _plan(keys, lambda out: load().sit_voronoi_plan(_d(cell), int(S), out, _d(rad)))
    if rc != OK:
        raise ValueError("voronoi_plan: a degenerate cell or no atom")
    plan["first_radius"], plan["growth"] = float(rad[0]), float(rad[1])
    return plan


COORDENV_SHAPES = ("S:1", "L:2", "TL:3", "T:4", "S:4", "T:5", "S:5", "O:6", "T:6", "PB:7", "C:8", "SA:8")   # library order


def coordenv_plan():
    """The plan of ``coordination_environments`` (``sit_coordenv_plan``): the caps, the workgroup, and the shape library as
    ``"symbols"``, ``"shape_n"`` and ``"shapes"`` (a list of ``[n, 3]`` unit vertices)."""
    sn, co = np.zeros(len(COORDENV_SHAPES), dtype=np.int32), np.zeros((len(COORDENV_SHAPES), 8, 3))
    keys = ["neighbour_cap", "vertex_cap", "face_cap", "coordination_cap", "max_n", "threads", "lds_bytes", "n_shapes"]
    rc, plan = _plan(keys, lambda out: load().sit_coordenv_plan(out, _ptr(sn), _d(co)))
    if rc != OK:
        raise ValueError("coordenv_plan")
    assert plan["n_shapes"] == len(COORDENV_SHAPES)
    plan["symbols"], plan["shape_n"] = list(COORDENV_SHAPES), [int(v) for v in sn]
    plan["shapes"] = [co[s, :sn[s]].copy() for s in range(len(COORDENV_SHAPES))]
    return plan


def release_cached_memory():
    """Returns the idle large device buffers the library keeps between contexts (sit_release_cached_memory)."""
    load().sit_release_cached_memory()


_STAGES = ("fill", "fit", "predict", "gram", "site_centers", "occupancy", "h2d")     # slots 0-6 of a block of sit_timers


def _settling(fn):
    """Deferred ``fill`` passes are collected before their output is read: a failed pass raises here (as the reference
    raises from inside its frame loop, landmark/helpers.pyx:76-92,116-118), a pass that outgrew its row buffers is run
    again at the rigorous width (``fill_result``).  Every method that reads rows or labels carries this decorator."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        if self._deferred:
            rc, _, err = self.fill_result()
            self._check(rc, err)
        return fn(self, *args, **kwargs)
    return wrapper


class HipContext(object):
    """One GPU-resident landmark-analysis context (thin, 1:1 over the C-ABI)."""

    def __init__(self, cell, device=None):
        self.lib = load()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        cell = _f64(cell).reshape(3, 3)
        # util/PBCCalculator.pyx:27-34 -- the inverse is numpy's, exactly as in the reference
        cell_inv = _f64(np.asarray(np.linalg.inv(cell.T)))
        self.cell = cell
        self.cell_centroid = np.sum(0.5 * cell, axis=0)
        h = _vp()
        rc = self.lib.sit_create(_d(cell), _d(cell_inv), int(device), C.byref(h))
        self._h = h
        self.device = int(device)
        if rc != OK:
            msg = self.message()
            self.close()
            raise RuntimeError("sit_create failed on device %d: %s (is a GPU visible?)" % (device, msg))
        self.D = self.S = self.M = self.F = self.N = self.K = self.A = 0
        self.frame0 = 0
        # who may trust the resident labels (site_trajectory.py): a counter of their rewrites and, when somebody has
        # looked, (version, content digest) of what is there
        self.labels_version = 0
        self.labels_digest = None
        self._deferred = 0                # sit_fill passes enqueued with defer and not collected yet
        self._last_fill = None

    def close(self):
        if getattr(self, "_h", None):
            self.lib.sit_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def message(self):
        m = self.lib.sit_last_message(self._h)
        return m.decode() if m else ""

    def _check(self, rc, err=None):
        if rc == OK:
            return
        if rc == RETRY:
            # (the methods below collect deferred passes - and repeat one that outgrew its row buffers - before they
            # read its output: _settling)
            raise RuntimeError("libsitator_hip: a deferred fill asked to be repeated (SIT_RETRY); call fill_result()")
        if rc in (E_INVALID, E_NOT_CONVERGED):
            raise ValueError(self.message())
        if rc in (E_HIP, E_CAPACITY):
            raise RuntimeError("libsitator_hip: %s" % self.message())
        raise errors.DeviceDomainError(rc, err.frame if err else -1, err.index if err else -1)

    def _check_index(self, rc):
        if rc == E_INVALID and self.message().startswith("index "):
            raise IndexError(self.message())
        self._check(rc)

    def _labels_rewritten(self):
        """Every call that rewrites the resident labels says so here (site_trajectory.py decides by it whose they are)."""
        self.labels_version += 1
        self.labels_digest = None

    def _records(self, width, call):
        """The int64 ``[n, width]`` records of ``call(cap, rec_ptr, n_byref)`` (which gives the status): asked for with room
        for ``1 << 16`` and, where there are more, again with room for all ``n``."""
        cap = 1 << 16
        while True:
            rec = np.empty((cap, width), dtype=np.int64)
            n = i64(0)
            self._check(call(cap, _i(rec), C.byref(n)))
            if n.value <= cap:
                return rec[:n.value]
            cap = int(n.value)

    def _frames(self, positions, A=None):
        """``(positions, F, A)``: a host ``[F, A, 3]`` array (of ``A`` atoms where that is given), or else ``None`` and the
        sizes of the resident frames."""
        if positions is None:
            return None, self.F, self.A
        positions = _f64(positions)
        assert positions.ndim == 3 and positions.shape[2] == 3 and A in (None, positions.shape[1])
        return positions, positions.shape[0], positions.shape[1]

    def _selection(self, positions, atoms):
        """``(positions, idx, F, n_sel)``: a host ``[F, n_sel, 3]`` array, or ``atoms`` as columns of the resident frames."""
        if positions is not None:
            positions, F, n_sel = self._frames(positions)
            return positions, None, F, n_sel
        idx = _i64(atoms).reshape(-1)
        return None, idx, self.F, len(idx)

    # -- PBCCalculator surface
    def wrap_points(self, pts):
        pts = _f64(pts)
        assert pts.ndim == 2 and pts.shape[1] == 3, "Points must be 3D"
        self._check(self.lib.sit_wrap_points(self._h, _d(pts), len(pts)))
        return pts

    def distances(self, pt1, pts2):
        pt1, pts2 = _f64(pt1), _f64(pts2)
        out = np.empty(len(pts2))
        self._check(self.lib.sit_distances(self._h, _d(pt1), _d(pts2), len(pts2), _d(out)))
        return out

    def average(self, pts, weights=None):
        pts = _f64(pts)
        w = _opt(_f64, weights)
        out = np.empty(3)
        self._check(self.lib.sit_average(self._h, _d(pts), _d(w), len(pts), _d(out)))
        return out

    @_settling
    def min_image(self, ref, pts):
        """``(moved points [n, 3], codes int32 [n])``: every ``pts[p]`` moved to its periodic image nearest ``ref[p]`` and
        the reference's code ``100 i + 10 j + k`` of that image (``sit_min_image``)."""
        ref = _f64(ref).reshape(-1, 3)
        pts = np.array(pts, dtype=np.float64).reshape(-1, 3)
        assert ref.shape == pts.shape
        code = np.zeros(len(pts), dtype=np.int32)
        self._check(self.lib.sit_min_image(self._h, _d(ref), _d(pts), len(pts), _ptr(code)))
        return pts, code

    def site_vertex_distances(self, centers, ref_static, verts):
        centers = _f64(centers); ref_static = _f64(ref_static); verts = _i64(verts)
        out = np.empty(verts.shape)
        self._check(self.lib.sit_site_vertex_distances(self._h, _d(centers), _d(ref_static), _i(verts), verts.shape[0],
                                                       verts.shape[1], len(ref_static), _d(out)))
        return out

    # -- residency
    def set_basis(self, ref_static, verts, vert_dists, midpoint, steepness, static_threshold):
        ref_static, verts, vert_dists = _f64(ref_static), _i64(verts), _f64(vert_dists)
        self.S = len(ref_static)
        self.D, self.V = verts.shape
        self._check(self.lib.sit_set_basis(self._h, _d(ref_static), self.S, _i(verts), _d(vert_dists),
                                           self.D, self.V, float(midpoint), float(steepness),
                                           float(static_threshold)))

    def frames_device_ptr(self):
        """Device address of the resident trajectory (sit_frames_device_ptr)."""
        p = C.c_void_p()
        self._check(self.lib.sit_frames_device_ptr(self._h, C.byref(p)))
        return p.value

    def _take_frames(self, frames, static_idx, mobile_idx, frame0):
        """The arrays of a trajectory as the library reads them; the context takes its sizes from them."""
        frames, static_idx, mobile_idx = _f64(frames), _i64(static_idx), _i64(mobile_idx)
        self.F, self.A = frames.shape[0], frames.shape[1]
        self.M = len(mobile_idx)
        self.N = self.F * self.M
        self.frame0 = int(frame0)
        return frames, static_idx, mobile_idx

    def set_frames(self, frames, static_idx, mobile_idx, frame0=0):
        frames, static_idx, mobile_idx = self._take_frames(frames, static_idx, mobile_idx, frame0)
        self._check(self.lib.sit_set_frames(self._h, _d(frames), self.F, self.A, _i(static_idx), len(static_idx),
                                            _i(mobile_idx), self.M, self.frame0))

    def upload_fill_fit(self, frames, static_idx, mobile_idx, frame0, dynamic_lattice_mapping, relaxed_lattice_checks,
                        check_for_zeros, fit_threshold):
        """``set_frames`` + ``fill`` + the first pass of ``fit_centers`` with the upload overlapped
        (``sit_upload_fill_fit``).  Returns ``(rc, n_all_zero, err, fitted)``."""
        frames, static_idx, mobile_idx = self._take_frames(frames, static_idx, mobile_idx, frame0)
        p = FillParams.make(dynamic_lattice_mapping, relaxed_lattice_checks, check_for_zeros, 1, 0, 1, 0.0)
        nz, err = i64(0), SitError()
        fitted = C.c_int(0)
        self._deferred = 0
        rc = self.lib.sit_upload_fill_fit(self._h, _d(frames), self.F, self.A, _i(static_idx), len(static_idx),
                                          _i(mobile_idx), self.M, self.frame0, C.byref(p), float(fit_threshold),
                                          C.byref(nz), C.byref(err), C.byref(fitted))
        return rc, nz.value, err, bool(fitted.value)

    def row_width(self):
        w = i64(0)
        self._check(self.lib.sit_row_width(self._h, C.byref(w)))
        return w.value

    # -- landmark vectors
    def fill(self, dynamic_lattice_mapping=False, relaxed_lattice_checks=False, check_for_zeros=True,
             assign=False, predict_threshold=0.0, store_rows=True, defer=False):
        """One pass over the resident frames (``sit_fill``).  ``assign``: the site assignment in the same pass (rows of up
        to four entries inside the fill kernel).  ``defer``: enqueue only; status, ``n_all_zero`` and the error come from
        ``fill_result()`` (or a later ``fill`` / ``synchronize``)."""
        p = FillParams.make(dynamic_lattice_mapping, relaxed_lattice_checks, check_for_zeros, store_rows, assign, 1,
                            predict_threshold, defer)
        nz, err = i64(0), SitError()
        if assign:
            self._labels_rewritten()
        self._last_fill = p
        rc = self.lib.sit_fill(self._h, C.byref(p), C.byref(nz), C.byref(err))
        self._deferred = self._deferred + 1 if (defer and rc == OK) else 0
        return rc, nz.value, err

    def fill_result(self):
        """Status, ``n_all_zero`` and error of the deferred passes in flight (waits for them; the first failure wins).
        A pass whose rows outgrew the buffers measured on the leading frames (``SIT_RETRY``) is run again, blocking."""
        nz, err = i64(0), SitError()
        rc = self.lib.sit_fill_result(self._h, C.byref(nz), C.byref(err))
        self._deferred = 0
        if rc == RETRY:
            p = self._last_fill
            p.defer = 0
            rc = self.lib.sit_fill(self._h, C.byref(p), C.byref(nz), C.byref(err))
        return rc, nz.value, err

    def static_seen(self, local_frame):
        seen = np.zeros(self.S, dtype=np.uint8)
        self._check(self.lib.sit_static_seen(self._h, int(local_frame), _ptr(seen)))
        return seen

    @_settling
    def rows_dense(self, row0=0, nrows=None):
        nrows = self.N - row0 if nrows is None else nrows
        out = np.empty((nrows, self.D))
        self._check(self.lib.sit_get_rows_dense(self._h, int(row0), int(nrows), _d(out)))
        return out

    @_settling
    def rows_sparse(self, row0=0, nrows=None):
        nrows = self.N - row0 if nrows is None else nrows
        W = self.row_width()
        nnz, idx, val = np.empty(nrows, dtype=np.int32), np.empty((W, nrows), dtype=np.int32), np.empty((W, nrows))
        self._check(self.lib.sit_get_rows_sparse(self._h, int(row0), int(nrows), _ptr(nnz), _ptr(idx), _d(val)))
        return nnz, idx, val

    def set_rows_dense(self, X):
        X = _f64(X)
        assert X.ndim == 2
        self._check(self.lib.sit_set_rows_dense(self._h, _d(X), X.shape[0], X.shape[1]))
        self.N, self.D = X.shape

    # -- DotProdClassifier
    def fit_reset(self):
        self._check(self.lib.sit_fit_reset(self._h))

    def fit_set_state(self, centers, counts):
        centers = _f64(centers).reshape(-1, self.D)
        counts = _i64(counts)
        self._check(self.lib.sit_fit_set_state(self._h, _d(centers), _i(counts), len(centers)))

    def fit_get_state(self):
        K = i64(0)
        self._check(self.lib.sit_fit_get_state(self._h, None, None, C.byref(K)))
        centers = np.empty((K.value, self.D))
        counts = np.empty(K.value, dtype=np.int64)
        if K.value:
            self._check(self.lib.sit_fit_get_state(self._h, _d(centers), _i(counts), C.byref(K)))
        return centers, counts

    @_settling
    def fit_push_stored_rows(self, threshold):
        self._check(self.lib.sit_fit_push_stored_rows(self._h, float(threshold)))

    def fit_push_dense_rows(self, rows, weights, threshold):
        rows = _f64(rows).reshape(-1, self.D)
        weights = _i64(weights)
        self._check(self.lib.sit_fit_push_dense_rows(self._h, _d(rows), _i(weights), len(rows), float(threshold)))

    @_settling
    def set_centers(self, matrix, normed):
        matrix = _f64(matrix).reshape(-1, self.D)
        self.K = len(matrix)
        self._check(self.lib.sit_set_centers(self._h, _d(matrix), self.K, int(bool(normed))))

    def prefault_assignments(self, n_rows):
        """Starts a thread that allocates the host arrays of the next fetching ``predict`` and touches their pages.  A
        read-back into a fresh 51-MB numpy array costs 2.5 ms, into one whose pages exist 1.0 ms (49 GB/s): the page
        faults, not the copy (scratch/d2h_probe.py); called ahead of the fill and the fit, the faults are taken on
        another core while the GPU works (ctypes calls release the GIL)."""
        import threading
        n = int(n_rows)
        box = {}

        def work():
            labels = np.empty(n, dtype=np.int64)
            confs = np.empty(n)
            labels[::512] = 0
            confs[::512] = 0.0
            box["arrays"] = (labels, confs)

        th = threading.Thread(target=work, daemon=True)
        th.start()
        self._prefault = (th, box, n)

    def _assignment_arrays(self):
        pf, self._prefault = getattr(self, "_prefault", None), None
        if pf is not None and pf[2] == self.N:
            pf[0].join()
            if "arrays" in pf[1]:
                return pf[1]["arrays"]
        return np.empty(self.N, dtype=np.int64), np.empty(self.N)

    @_settling
    def predict(self, threshold, fetch=True):
        self._labels_rewritten()
        counts = np.zeros(self.K, dtype=np.int64)
        labels, confs = self._assignment_arrays() if fetch else (None, None)
        self._check(self.lib.sit_predict(self._h, float(threshold), _i(labels), _d(confs), _i(counts)))
        return labels, confs, counts

    @_settling
    def assignments(self):
        labels, confs, counts = np.empty(self.N, dtype=np.int64), np.empty(self.N), np.zeros(self.K, dtype=np.int64)
        self._check(self.lib.sit_get_assignments(self._h, _i(labels), _d(confs), _i(counts)))
        return labels, confs, counts

    @_settling
    def count_zero_rows(self):
        """(number of all-zero rows, index of the first one or -1)."""
        n, first = i64(0), i64(0)
        self._check(self.lib.sit_count_zero_rows(self._h, C.byref(n), C.byref(first)))
        return n.value, first.value

    # -- mcl support
    @_settling
    def gram(self):
        G, seen = np.empty((self.D, self.D)), np.empty(self.D, dtype=np.int64)
        self._check(self.lib.sit_gram(self._h, _d(G), _i(seen)))
        return G, seen

    @_settling
    def gram_limbs(self):
        """The Gram matrix as exact integers (hi, lo) in units of 2^-80 (see ``exact_sum_across``), and ``seen``."""
        hi, lo = np.empty((self.D, self.D), dtype=np.uint64), np.empty((self.D, self.D), dtype=np.uint64)
        seen = np.empty(self.D, dtype=np.int64)
        self._check(self.lib.sit_gram_limbs(self._h, _ptr(hi), _ptr(lo), _i(seen)))
        return hi, lo, seen

    @_settling
    def weighted_row_sums_limbs(self, K, weighted=True):
        n = K * self.D + K
        hi, lo = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
        self._check(self.lib.sit_weighted_row_sums_limbs(self._h, int(weighted), int(K), _ptr(hi), _ptr(lo)))
        return hi, lo

    @_settling
    def best_match(self, c):
        c = _f64(c)
        row, dot, nrm = i64(0), C.c_double(0), C.c_double(0)
        self._check(self.lib.sit_best_match(self._h, _d(c), C.byref(row), C.byref(dot), C.byref(nrm)))
        return row.value, dot.value, nrm.value

    @_settling
    def best_match_groups(self, group_of_dim, cvec, G):
        """``best_match`` for ``G`` centres with disjoint supports in one pass: (rows, dots, norms), each ``[G]``."""
        grp = _i32(group_of_dim)
        cvec = _f64(cvec)
        assert grp.shape == (self.D,) and cvec.shape == (self.D,)
        rows, dots, nrms = np.empty(G, dtype=np.int64), np.empty(G), np.empty(G)
        self._check(self.lib.sit_best_match_groups(self._h, _ptr(grp), _d(cvec), G, _i(rows), _d(dots), _d(nrms)))
        return rows, dots, nrms

    @_settling
    def weighted_row_sums(self, K, weighted=True):
        sums, wsum = np.empty((K, self.D)), np.empty(K)
        self._check(self.lib.sit_weighted_row_sums(self._h, int(weighted), int(K), _d(sums), _d(wsum)))
        return sums, wsum

    # -- site centres / occupancy
    @_settling
    def site_anchors(self, K, weighted):
        wmax, first, pts = np.empty(K), np.empty(K, dtype=np.int64), np.empty((K, 3))
        self._check(self.lib.sit_site_anchors(self._h, int(weighted), int(K), _d(wmax), _i(first), _d(pts)))
        return wmax, first, pts

    @_settling
    def site_sums(self, K, weighted, anchors):
        anchors = _f64(anchors)
        sums = np.empty((K, 4))
        self._check(self.lib.sit_site_sums(self._h, int(weighted), int(K), _d(anchors), _d(sums)))
        return sums

    @_settling
    def check_occupancy(self, K, max_per_site):
        a, b, c = i64(0), i64(0), i64(0)
        err = SitError()
        rc = self.lib.sit_check_occupancy(self._h, int(K), int(max_per_site), C.byref(a), C.byref(b), C.byref(c),
                                          C.byref(err))
        return rc, a.value, b.value, c.value, err

    def set_assignments(self, labels, confs=None, frame0=0):
        self._labels_rewritten()
        labels = _i64(labels)
        F, M = labels.shape
        c = _opt(_f64, confs)
        self._check(self.lib.sit_set_assignments(self._h, _i(labels), _d(c), F, M, int(frame0)))
        self.F, self.M, self.N, self.frame0 = F, M, F * M, int(frame0)

    @_settling
    def site_counts(self, K):
        counts = np.zeros(int(K), dtype=np.int64)
        self._check(self.lib.sit_site_counts(self._h, int(K), _i(counts)))
        return counts

    @_settling
    def cooccupancy(self, K):
        """``bool[K, K]``: entry (a, b) says whether some resident frame has one ion on site a and one on site b
        (``sit_cooccupancy``; at most 16384 sites)."""
        K = int(K)
        co = np.zeros((K, K), dtype=np.uint8)
        rc = self.lib.sit_cooccupancy(self._h, K, _ptr(co))
        # a label beyond the sites: the reference's connmat[site, frame] raises this (MergeSitesByThreshold.py:70)
        self._check_index(rc)
        return co.view(np.bool_)

    JUMP_NONE = -(1 << 63)

    @_settling
    def jump_sources(self, unknown_as_jump=False, last_known_in=None):
        src, last_out = np.empty((self.F, self.M), dtype=np.int64), np.empty(self.M, dtype=np.int64)
        lin = _opt(_i64, last_known_in)
        self._check(self.lib.sit_jump_sources(self._h, int(unknown_as_jump), _i(lin), _i(src), _i(last_out)))
        return src, last_out

    @_settling
    def jump_list(self, unknown_as_jump=False, last_known_in=None):
        """Jumps as an ``[n, 4]`` array of (frame, mobile atom, from site, to site), frame-major, and the last known
        site of every ion after this context's frames."""
        last_out = np.empty(self.M, dtype=np.int64)
        lin = _opt(_i64, last_known_in)
        rec = self._records(4, lambda cap, rec, n: self.lib.sit_jump_list(self._h, int(unknown_as_jump), _i(lin), cap, rec, n,
                                                                          _i(last_out)))
        order = np.lexsort((rec[:, 1], rec[:, 0]))
        return rec[order], last_out

    @_settling
    def jump_analysis(self, K, last_known_in=None, time_at_current_in=None):
        n_ij = np.empty((K, K)); tsum = np.empty((K, K)); tn = np.empty((K, K), dtype=np.int64)
        total = np.empty(K, dtype=np.int64); nprob = i64(0)
        lout = np.empty(self.M, dtype=np.int64); tout = np.empty(self.M, dtype=np.int64)
        lin = _opt(_i64, last_known_in)
        tin = _opt(_i64, time_at_current_in)
        rc = self.lib.sit_jump_analysis(self._h, int(K), _i(lin), _i(tin), _d(n_ij), _d(tsum), _i(tn), _i(total),
                                        C.byref(nprob), _i(lout), _i(tout))
        # a label beyond the site tables: the reference's fancy indexing raises this (dynamics/JumpAnalysis.py:75-88)
        self._check_index(rc)
        return n_ij, tsum, tn, total, nprob.value, lout, tout

    @_settling
    def assign_last_known(self, frame_threshold, last_known_in=None, time_unknown_in=None, out=None):
        """``out``: a C-contiguous int64 [F, M] array that receives the new labels (else a fresh one)."""
        labels = np.empty((self.F, self.M), dtype=np.int64) if out is None else out
        assert labels.dtype == np.int64 and labels.flags.c_contiguous and labels.shape == (self.F, self.M)
        self._labels_rewritten()            # the kernel rewrites the resident labels in place
        fmax = np.zeros(max(self.F, 1), dtype=np.int32)
        st = np.zeros(3, dtype=np.int64)
        lout = np.empty(self.M, dtype=np.int64); tout = np.empty(self.M, dtype=np.int64)
        lin = _opt(_i64, last_known_in)
        tin = _opt(_i64, time_unknown_in)
        self._check(self.lib.sit_assign_last_known(self._h, int(frame_threshold), _i(lin), _i(tin), _i(labels), _ptr(fmax),
                                                   _i(st), _i(lout), _i(tout)))
        return labels, fmax[:self.F], st, lout, tout

    # -- ReplaceUnassignedPositions: the resident labels are read, never written (labels_version stays)
    ENDS_NONE = -(1 << 63)

    def _halo_pair(self, before_in, after_in):
        if (before_in is None) != (after_in is None):
            raise ValueError("before_in and after_in come as a pair")
        if before_in is None:
            return None, None
        b, a = _i64(before_in), _i64(after_in)
        assert b.shape == (self.M,) and a.shape == (self.M,)
        return b, a

    @_settling
    def label_ends(self):
        """Per ion the first and the last label != -1 of this context's frames (``ENDS_NONE`` where it has none)."""
        first = np.full(self.M, self.ENDS_NONE, dtype=np.int64)
        last = np.full(self.M, self.ENDS_NONE, dtype=np.int64)
        self._check(self.lib.sit_label_ends(self._h, _i(first), _i(last)))
        return first, last

    @_settling
    def replace_unassigned(self, mode, before_in=None, after_in=None):
        """The labels with every -1 replaced by the nearest known label before it (``mode`` 0) or after it (1);
        ``before_in`` / ``after_in`` ([M]): what holds before the first and after the last frame (default -1)."""
        b, a = self._halo_pair(before_in, after_in)
        out = np.empty((self.F, self.M), dtype=np.int64)
        self._check(self.lib.sit_replace_unassigned(self._h, int(mode), _i(b), _i(a), _i(out)))
        return out

    @_settling
    def unknown_runs(self, before_in=None, after_in=None):
        """``(records, n_positions)``: every maximal run of -1 as (ion, start, end, before, after, pos_offset), ion-major
        and by start; start / end are global frame numbers (``sit_unknown_runs``)."""
        b, a = self._halo_pair(before_in, after_in)
        npos = i64(0)
        rec = self._records(6, lambda cap, rec, n: self.lib.sit_unknown_runs(self._h, _i(b), _i(a), cap, rec, n, C.byref(npos)))
        return rec, int(npos.value)

    @_settling
    def replace_closer(self, records, centers, positions):
        """The labels with the runs of ``records`` (as ``unknown_runs`` gives them) filled by the closer-site rule;
        ``positions`` [n_positions, 3]: the ion's real-space position at every frame of the runs with an offset.  A site
        beyond ``centers`` raises ``IndexError``, any other record that does not fit the context ``ValueError``."""
        records = _i64(records).reshape(-1, 6)
        centers = _f64(centers).reshape(-1, 3)
        positions = _f64(positions).reshape(-1, 3)
        out = np.empty((self.F, self.M), dtype=np.int64)
        rc = self.lib.sit_replace_closer(self._h, _i(records), len(records), _d(centers), len(centers), _d(positions),
                                         len(positions), _i(out))
        # a label beyond the sites: the reference's centers[before_site] raises this (ReplaceUnassignedPositions.py:75)
        self._check_index(rc)
        return out

    @_settling
    def running_mode(self, wleft, wright, threshold, replace_unknown, n_sites=0):
        """The smoothed labels, and (``n_sites`` > 0) how often every site occurs among them."""
        out = np.empty((self.F, self.M), dtype=np.int64)
        counts = np.zeros(int(n_sites), dtype=np.int64) if n_sites > 0 else None
        self._check(self.lib.sit_running_mode(self._h, int(wleft), int(wright), int(threshold), int(replace_unknown), _i(out),
                                              int(n_sites), _i(counts)))
        return (out, counts) if counts is not None else out

    def recenter(self, arr, masses, factors, add3=None):
        assert arr.dtype == np.float64 and arr.flags.c_contiguous and arr.ndim == 3 and arr.shape[2] == 3
        masses = _f64(masses); factors = _f64(factors)
        a3 = _opt(_f64, add3)
        self._check(self.lib.sit_recenter(self._h, _d(arr), arr.shape[0], arr.shape[1], _d(masses), _d(factors), _d(a3)))

    def recenter_resident(self, masses, factors, add3=None):
        """Recentre the frames resident after ``set_frames`` in place on the device (``sit_recenter_resident``)."""
        masses = _f64(masses); factors = _f64(factors)
        assert len(masses) == self.A and len(factors) == self.A
        a3 = _opt(_f64, add3)
        self._check(self.lib.sit_recenter_resident(self._h, _d(masses), _d(factors), _d(a3)))

    # -- AverageVibrationalFrequency: reads frames only (labels_version, rows and labels stay)
    def speed_spectrum(self, freqs, fmask, positions=None, atoms=None, workspace_bytes=0, spectrum=False, speeds=False):
        """Per selected atom ``(avg, band_power, spectrum, speeds)`` of the speeds ``|x[t+1] - x[t]|`` (``sit_speed_spectrum``):
        the power-weighted mean of ``freqs`` over the bins where ``fmask`` holds, the power in them, and - where asked for,
        else ``None`` - the complex bins ``[n_sel, n // 2 + 1]`` of ``rfft(speeds)`` and the speeds ``[n_sel, n]``,
        ``n = F - 1``.  ``positions``: a host ``[F, n_sel, 3]`` float64 array; without it ``atoms`` names columns of the
        frames resident after ``set_frames``.  ``workspace_bytes``: cap on the device buffers of a batch of atoms (0: the
        default of 1 GiB)."""
        positions, idx, F, n_sel = self._selection(positions, atoms)
        nbins = max(F - 1, 0) // 2 + 1
        freqs = _f64(freqs)
        fmask = np.ascontiguousarray(fmask, dtype=np.uint8)
        assert freqs.shape == (nbins,) and fmask.shape == (nbins,)
        avg, power = np.empty(n_sel), np.empty(n_sel)
        spec = np.empty((n_sel, nbins), dtype=np.complex128) if spectrum else None
        spd = np.empty((n_sel, max(F - 1, 0))) if speeds else None
        self._check(self.lib.sit_speed_spectrum(self._h, _d(positions), int(F), _i(idx), int(n_sel), _d(freqs), _ptr(fmask),
                                                int(workspace_bytes), _d(avg), _d(power), _ptr(spec), _d(spd)))
        return avg, power, spec, spd

    # -- MeanSquaredDisplacement: reads frames only (labels_version, rows and labels stay)
    def msd(self, positions=None, atoms=None, unwrap=True, max_lag=None, lags=None, collective=False, workspace_bytes=0,
            r4=False, images=False):
        """``(msd [n_sel, 3, n_lags], r4 [n_sel, n_lags], coll [3, n_lags], images int32 [n_sel, F, 3], max_residual)`` of
        ``sit_msd``; whatever was not asked for is ``None``.  ``positions``: a host ``[F, n_sel, 3]`` float64 array; without
        it ``atoms`` names columns of the frames resident after ``set_frames``.  ``lags=None``: all lags ``0 .. max_lag``
        (``None``: ``F // 2``) through the transform; otherwise the lags listed, by direct sums, with ``r4`` on request.
        ``unwrap``: under the context's cell.  ``workspace_bytes``: cap on the device buffers of a batch of atoms (0: the
        default of 1 GiB).  A lag or an atom out of range, and any other argument that does not fit, raises
        ``ValueError``."""
        positions, idx, F, n_sel = self._selection(positions, atoms)
        if lags is None:
            lag_arr = None
            max_lag = F // 2 if max_lag is None else int(max_lag)
            n_lags = max(max_lag, 0) + 1
            if r4:
                raise ValueError("msd: the fourth moment comes with an explicit lag list only")
        else:
            lag_arr = _i64(lags).reshape(-1)
            max_lag, n_lags = 0, len(lag_arr)
        out = np.zeros((n_sel, 3, n_lags))
        out4 = np.zeros((n_sel, n_lags)) if r4 else None
        coll = np.zeros((3, n_lags)) if collective else None
        img = np.zeros((n_sel, max(F, 0), 3), dtype=np.int32) if images else None
        res = C.c_double(0.0)
        self._check(self.lib.sit_msd(self._h, _d(positions), int(F), _i(idx), int(n_sel), int(bool(unwrap)), int(max_lag), _i(lag_arr),
                                     int(n_lags), int(bool(collective)), int(workspace_bytes), _d(out), _d(out4), _d(coll), _ptr(img),
                                     C.byref(res)))
        return out, out4, coll, img, res.value

    # -- GenerateClampedTrajectory: reads labels and frames only (labels_version, rows and labels stay)
    @_settling
    def clamp_trajectory(self, role, fixed_pos, centers, wrap, pass_through_unassigned, positions=None, workspace_bytes=0):
        """``float64[F, A, 3]`` (``sit_clamp_trajectory``): per atom, by ``role[a]``, its real position (-1),
        ``fixed_pos[a]`` (-2) or the centre of the site that column ``role[a]`` of the resident labels names - as given
        with ``wrap``, else its periodic image nearest the atom's real position.  ``positions``: a host ``[F, A, 3]``
        float64 array; without it the frames resident after ``set_frames`` are read (none are needed with ``wrap``, no
        role -1 and no pass-through).  ``workspace_bytes``: cap on the device buffers of a chunk of frames (0: the default
        of 1 GiB).  An unassigned label without ``pass_through_unassigned`` raises ``errors.UnassignedClampError`` (a
        ``RuntimeError``; ``.first_unassigned`` = the smallest frame * M + column), a label ``>= len(centers)``
        ``IndexError``, any other argument that does not fit the context ``ValueError``."""
        role = _i32(role).reshape(-1)
        A = len(role)
        fixed_pos = _f64(fixed_pos).reshape(A, 3)
        centers = _f64(centers).reshape(-1, 3)
        positions, F, _ = self._frames(positions, A)
        out = np.empty((F, A, 3))
        first = i64(-1)
        rc = self.lib.sit_clamp_trajectory(self._h, _d(positions), int(F), int(A), _ptr(role), _d(fixed_pos), _d(centers), len(centers),
                                           int(bool(wrap)), int(bool(pass_through_unassigned)), int(workspace_bytes), _d(out),
                                           C.byref(first))
        if rc == E_UNASSIGNED:
            raise errors.UnassignedClampError(first.value)
        # a label beyond the sites: the reference's centers_c[at_site] reads past the table (GenerateClampedTrajectory.pyx:99)
        self._check_index(rc)
        return out

    # -- per-site point clouds: reads labels and frames only (labels_version, rows and labels stay)
    @_settling
    def group_by_site(self, K, positions=None, mobile_idx=None, workspace_bytes=0):
        """``offsets`` int64 ``[K + 1]`` of a stable grouping of the assigned entries ``frame * M + column`` of the resident
        labels by site (``sit_group_by_site``): sites ascending, entries ascending inside a site - the order of
        ``real_traj[:, mobile_mask][traj == site]``.  ``positions``: a host ``[F, A, 3]`` float64 array with ``mobile_idx``
        ``[M]`` naming the atoms of the label columns; without it the frames resident after ``set_frames`` are read.  The
        grouping stays on the device (``grouped_fetch``, ``grouped_bucket_averages``, ``grouped_recenter_step``) until the
        labels are rewritten.  A label ``>= K`` raises ``IndexError``, anything else that does not fit ``ValueError``."""
        K = int(K)
        offsets = np.zeros(K + 1, dtype=np.int64)
        positions, F, A = self._frames(positions)
        midx = _i64(mobile_idx).reshape(-1) if positions is not None else None
        M = self.M if midx is None else len(midx)
        rc = self.lib.sit_group_by_site(self._h, _d(positions), int(F), int(A), _i(midx), int(M), K, int(workspace_bytes),
                                        _i(offsets))
        self._check_index(rc)
        return offsets

    @_settling
    def grouped_fetch(self, first, n, points=True, confidences=False, entries=False):
        """``(points [n, 3], confidences [n], entries [n])`` of the elements ``[first, first + n)`` of the grouping, ``None``
        for what was not asked for.  ``ValueError`` ("stale ...") once the labels have been rewritten."""
        n = int(n)
        pts = np.empty((n, 3)) if points else None
        cf = np.empty(n) if confidences else None
        en = np.empty(n, dtype=np.int64) if entries else None
        self._check(self.lib.sit_grouped_fetch(self._h, int(first), n, _d(pts), _d(cf), _i(en)))
        return pts, cf, en

    @_settling
    def grouped_bucket_averages(self, K, n_avg, weighted):
        """``(centers [K, n_avg, 3], anchors [K, n_avg])``: ``PBCCalculator.average`` of the elements of every site at ranks
        ``i, i + n_avg, ...`` (``sit_grouped_bucket_averages``); NaN / -1 for sites of at most ``n_avg`` elements."""
        out = np.empty((int(K), int(n_avg), 3))
        anchors = np.empty((int(K), int(n_avg)), dtype=np.int64)
        self._check(self.lib.sit_grouped_bucket_averages(self._h, int(n_avg), int(bool(weighted)), _d(out), _i(anchors)))
        return out, anchors

    @_settling
    def grouped_recenter_step(self, i, n_recenterings, out):
        """Step ``i`` of the cumulative recentring of every site's points (``sit_grouped_recenter_step``) into ``out``
        ``[N, 3]`` (float64, C-contiguous; ``None``: not copied back).  An empty site raises ``IndexError``."""
        assert out is None or (out.ndim == 2 and out.shape[1] == 3)
        self._check_index(self.lib.sit_grouped_recenter_step(self._h, int(i), int(n_recenterings), _d(out)))
        return out

    @_settling
    def grouped_hull_volumes(self, K, vertex_mask=False):
        """``(volumes [K], status int32 [K], n_facets int32 [K], vertex_mask uint8 [N] or None)``: the convex hull of every
        site's points in the working copy as the last ``grouped_recenter_step`` left it (``sit_grouped_hull_volumes``).
        ``status`` 0: closed, the volume is the hull's; 1: fewer than 4 points; 2: an uncertain orientation test; 3: beyond
        the capacity of ``hull_plan()``; 4: not closed - the volume is NaN for all of these.  ``ValueError`` before step 0
        and for a stale grouping."""
        info = self.group_info()
        if int(K) != info["n_sites"]:
            raise ValueError("grouped_hull_volumes: K is not the number of sites of the grouping")
        vols, status, nf = np.empty(int(K)), np.empty(int(K), dtype=np.int32), np.empty(int(K), dtype=np.int32)
        mask = np.zeros(info["n_grouped"], dtype=np.uint8) if vertex_mask else None
        self._check(self.lib.sit_grouped_hull_volumes(self._h, _d(vols), _ptr(status), _ptr(nf), _ptr(mask)))
        return vols, status, nf, mask

    @_settling
    def grouped_work_fetch(self, first, n):
        """``points [n, 3]`` of the elements ``[first, first + n)`` of the recentred working copy
        (``sit_grouped_work_fetch``)."""
        n = int(n)
        pts = np.empty((n, 3))
        self._check(self.lib.sit_grouped_work_fetch(self._h, int(first), n, _d(pts)))
        return pts

    def group_info(self):
        v = np.zeros(8)
        self.lib.sit_group_info(self._h, _d(v), 8)
        return {"n_grouped": int(v[0]), "n_sites": int(v[1]), "chunks": int(v[2]), "lds": bool(v[3]), "group_ms": float(v[4]),
                "bucket_avg_ms": float(v[5]), "recenter_ms": float(v[6]), "hull_ms": float(v[7])}

    # -- DiffusionPathwayAnalysis: reads nothing of the context but its cell
    @_settling
    def pathway_components(self, conn, centers, n_images=27, codes=False):
        """``(root int32 [n_images * K], rounds, code int32 [K, K] or None)`` of the site graph ``conn`` ``[K, K]`` (non-zero:
        connected) under the context's cell (``sit_pathway_components``): per node ``image * K + site`` of the 3 x 3 x 3
        supercell (``n_images`` 27; 1: the plain graph) the lowest node index of its connected component, the rounds the
        labelling took, and with ``codes`` the image code of every connected pair.  More than 16384 sites: ``ValueError``."""
        conn = np.ascontiguousarray(conn, dtype=np.uint8)
        assert conn.ndim == 2 and conn.shape[0] == conn.shape[1]
        K = conn.shape[0]
        centers = _f64(centers).reshape(-1, 3)
        assert len(centers) == K
        root = np.empty(int(n_images) * K, dtype=np.int32)
        code = np.empty((K, K), dtype=np.int32) if codes else None
        rounds = i64(0)
        self._check(self.lib.sit_pathway_components(self._h, K, _ptr(conn), _d(centers), int(n_images), _ptr(code), _ptr(root),
                                                    C.byref(rounds)))
        return root, int(rounds.value), code

    # -- MergeSitesByBarrier: reads nothing of the context but its cell
    @_settling
    def barrier_energies(self, static_pos, eps, sigma, rc, centers, pairs, coeffs, threshold, energies=True, codes=False):
        """``(energies [P, n] or None, verdict uint8 [P, 3], code int32 [P] or None)`` (``sit_barrier_energies``): per pair
        ``(i, j)`` of ``pairs`` ``[P, 2]`` the energy of one mobile atom at the ``n`` points ``vector * coeffs[m] + centers[i]``
        (``vector``: from ``centers[i]`` to the nearest image of ``centers[j]``) among the atoms ``static_pos`` ``[S, 3]`` and
        all their periodic images, under the truncated and shifted 12-6 potential of ``eps`` / ``sigma`` ``[S]`` and ``rc``;
        ``verdict``: the maximum is interior, forward barrier <= ``threshold``, backward barrier <= ``threshold``; ``code``:
        the ``min_image`` code of the pair.  Anything that does not fit raises ``ValueError``."""
        static_pos = _f64(static_pos).reshape(-1, 3)
        eps, sigma = _f64(eps).reshape(-1), _f64(sigma).reshape(-1)
        assert len(eps) == len(static_pos) == len(sigma)
        centers = _f64(centers).reshape(-1, 3)
        pairs = _i32(pairs).reshape(-1, 2)
        coeffs = _f64(coeffs).reshape(-1)
        P, n = len(pairs), len(coeffs)
        en = np.empty((P, n)) if energies else None
        verdict = np.zeros((P, 3), dtype=np.uint8)
        code = np.zeros(P, dtype=np.int32) if codes else None
        self._check(self.lib.sit_barrier_energies(self._h, _d(static_pos), _d(eps), _d(sigma), len(static_pos), float(rc), _d(centers),
                                                  len(centers), _ptr(pairs), P, _d(coeffs), n, float(threshold), _d(en),
                                                  _ptr(verdict), _ptr(code)))
        return en, verdict, code

    # -- VoronoiSiteGenerator: reads nothing of the context but its cell
    @_settling
    def voronoi_nodes(self, static_pos, tau):
        """``{"centers" [n, 3], "radii" [n], "vertices" (list of n int arrays), "status" int32 [S], "nbr_count" int32 [S],
        "info" dict}`` (``sit_voronoi_nodes``, size call then fill call): the periodic Voronoi nodes of ``static_pos`` ``[S, 3]``
        under the context's cell for the tolerance ``tau``.  Unless every status is 0 and the merge unambiguous there are no nodes."""
        static_pos = _f64(static_pos).reshape(-1, 3)
        S = len(static_pos)
        status, nbr = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
        info = np.zeros(8)
        nn, ni = i64(0), i64(0)
        head = (self._h, _d(static_pos), S, float(tau))
        tail = (_ptr(status), _ptr(nbr), _d(info))
        self._check(self.lib.sit_voronoi_nodes(*head, 0, 0, C.byref(nn), C.byref(ni), None, None, None, None, *tail))
        n, m = int(nn.value), int(ni.value)
        centers, radii = np.zeros((n, 3)), np.zeros(n)
        offsets, indices = np.zeros(n + 1, dtype=np.int64), np.zeros(max(m, 1), dtype=np.int32)
        self._check(self.lib.sit_voronoi_nodes(*head, n, m, C.byref(nn), C.byref(ni), _d(centers), _d(radii), _i(offsets),
                                               _ptr(indices), *tail))
        assert int(nn.value) == n and int(ni.value) == m
        keys = ["rounds", "final_radius", "max_neighbours", "records", "kernel_ms", "first_radius", "merge_status"]
        out_info = {k: (float(v) if k in ("final_radius", "kernel_ms", "first_radius") else int(v)) for k, v in zip(keys, info)}
        return {"centers": centers, "radii": radii, "vertices": [indices[offsets[j]:offsets[j + 1]].copy() for j in range(n)],
                "status": status, "nbr_count": nbr, "info": out_info}

    # -- SiteCoordinationEnvironment: reads nothing of the context but its cell
    @_settling
    def coordination_environments(self, static_pos, centers, tau=1e-6, distance_cutoff=1.4, angle_cutoff=0.3, max_csm=8.0):
        """``{"status", "flags", "n", "shape" int32 [K], "vertices" (list of K int arrays: static indices of the coordinating
        images, ordered by distance, static index, image), "norm_distance", "norm_angle" (lists of K arrays), "csm_best" [K],
        "csm_all" [K, 3], "confidence" [K], "info" dict}`` (``sit_coordination_environments``, size call then fill call) for the
        sites ``centers`` ``[K, 3]`` among ``static_pos`` ``[S, 3]`` under the context's cell."""
        static_pos, centers = _f64(static_pos).reshape(-1, 3), _f64(centers).reshape(-1, 3)
        S, K = len(static_pos), len(centers)
        i32 = lambda: np.zeros(max(K, 1), dtype=np.int32)
        status, flags, n, shape = i32(), i32(), i32(), i32()
        best, call, conf, info = np.zeros(max(K, 1)), np.zeros((max(K, 1), 3)), np.zeros(max(K, 1)), np.zeros(8)
        ni = i64(0)
        head = (self._h, _d(static_pos), S, _d(centers), K, float(tau), float(distance_cutoff), float(angle_cutoff), float(max_csm))
        per = (_ptr(status), _ptr(flags), _ptr(n))
        tail = (_ptr(shape), _d(best), _d(call), _d(conf), _d(info))
        self._check(self.lib.sit_coordination_environments(*head, 0, C.byref(ni), *per, None, None, None, None, *tail))
        computed = int(info[7])
        m = int(ni.value)
        offsets, indices = np.zeros(K + 1, dtype=np.int64), np.zeros(max(m, 1), dtype=np.int32)
        nd, na = np.zeros(max(m, 1)), np.zeros(max(m, 1))
        self._check(self.lib.sit_coordination_environments(*head, m, C.byref(ni), *per, _i(offsets), _ptr(indices), _d(nd), _d(na),
                                                           *tail))
        assert int(ni.value) == m
        keys = ["rounds", "final_radius", "max_neighbours", "max_n", "cell_ms", "csm_ms", "first_radius", "fill_computed"]
        out_info = {k: (int(v) if k in ("rounds", "max_neighbours", "max_n", "fill_computed") else float(v)) for k, v in zip(keys, info)}
        out_info["size_computed"] = computed
        cut = lambda a: [a[offsets[j]:offsets[j + 1]].copy() for j in range(K)]
        return {"status": status[:K], "flags": flags[:K], "n": n[:K], "shape": shape[:K], "vertices": cut(indices), "norm_distance": cut(nd),
                "norm_angle": cut(na), "csm_best": best[:K], "csm_all": call[:K], "confidence": conf[:K], "info": out_info}

    # -- SOAP descriptors: soap_vectors reads nothing of the context but its cell, soap_site_averages labels and frames only
    def _soap_args(self, soap):
        """The tail of scalars and tables the SOAP entry points share, from a ``soap`` dict (``site_descriptors.soap_tables``)."""
        alpha, beta = _f64(soap["alpha"]), _f64(soap["beta"])
        L, n = int(soap["l_max"]) + 1, int(soap["n_max"])
        assert alpha.shape == (L, n) and beta.shape == (L, n, n)
        return (float(soap["cutoff"]), float(soap["cutoff_transition_width"]), float(soap["atom_sigma"]), int(soap["n_species"]), n,
                L - 1, int(bool(soap["crossover"])), _d(alpha), _d(beta), int(soap["n_dim"]))

    @_settling
    def soap_vectors(self, static_pos, species_idx, centers, soap, nbr_count=False):
        """``(out [P, n_dim], nbr_count int32 [P] or None)`` (``sit_soap_vectors``): the SOAP power spectrum of every centre among
        the atoms ``static_pos`` ``[S, 3]`` and all their periodic images under the context's cell; ``species_idx`` ``[S]``: the
        index of an atom's species in the environment list, -1 for an atom outside it.  ``soap``: the dict of
        ``site_descriptors.soap_tables``.  Beyond a capacity ``RuntimeError``, anything else that does not fit ``ValueError``."""
        static_pos = _f64(static_pos).reshape(-1, 3)
        species_idx = _i32(species_idx).reshape(-1)
        assert len(species_idx) == len(static_pos)
        centers = _f64(centers).reshape(-1, 3)
        tail = self._soap_args(soap)
        P = len(centers)
        out = np.zeros((P, int(soap["n_dim"])))
        cnt = np.zeros(P, dtype=np.int32) if nbr_count else None
        self._check(self.lib.sit_soap_vectors(self._h, _d(static_pos), _ptr(species_idx), len(static_pos), _d(centers), P, *tail,
                                              _d(out), _ptr(cnt)))
        return out, cnt

    @_settling
    def soap_site_averages(self, K, static_idx, species_idx, mobile_idx, soap, stepsize=1, averaging=None, avg_descriptors_per_site=None,
                           positions=None, workspace_bytes=0):
        """``(descs [R, n_dim], counts [K], nr_of_descs [K], info)`` (``sit_soap_site_averages``, size call then fill call): the
        averaged SOAP vectors of ``SOAPDescriptorAverages`` on the resident labels; ``positions``: a host ``[F, A, 3]`` float64
        array, without it the frames resident after ``set_frames`` are read.  A label ``>= K`` raises ``IndexError``."""
        static_idx, mobile_idx = _i64(static_idx).reshape(-1), _i64(mobile_idx).reshape(-1)
        species_idx = _i32(species_idx).reshape(-1)
        assert len(species_idx) == len(static_idx)
        positions, F, A = self._frames(positions)
        K = int(K)
        tail = self._soap_args(soap)
        counts, nr = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        info = np.zeros(4)
        n_rows = i64(0)
        head = (self._h, _d(positions), int(F), int(A), _i(static_idx), _ptr(species_idx), len(static_idx), _i(mobile_idx),
                len(mobile_idx), K, int(stepsize), int(averaging or 0), int(avg_descriptors_per_site or 0))
        self._check_index(self.lib.sit_soap_site_averages(*head, *tail, int(workspace_bytes), 0, C.byref(n_rows), _i(counts), _i(nr),
                                                          None, _d(info)))
        R = int(n_rows.value)
        descs = np.zeros((R, int(soap["n_dim"])))
        self._check_index(self.lib.sit_soap_site_averages(*head, *tail, int(workspace_bytes), R, C.byref(n_rows), _i(counts), _i(nr),
                                                          _d(descs), _d(info)))
        assert int(n_rows.value) == R
        return descs, counts, nr, {"kernel_ms": float(info[0]), "contributors": int(info[1]), "chunks": int(info[2]),
                                   "averaging": int(info[3])}

    # -- SiteTypeAnalysis: PCA statistics and density-peak clustering; they read nothing of the context but its device
    @_settling
    def pca_covariance(self, X):
        """``(mean [D], cov [D, D])`` of the rows ``X`` ``[N, D]`` (``sit_pca_covariance``): ``cov`` has the divisor
        ``max(N - 1, 1)``.  Beyond a capacity ``RuntimeError``, anything else that does not fit ``ValueError``."""
        X = _f64(X)
        assert X.ndim == 2
        N, D = X.shape
        mean, cov = np.zeros(D), np.zeros((D, D))
        self._check(self.lib.sit_pca_covariance(self._h, _d(X), N, D, _d(mean), _d(cov)))
        return mean, cov

    @_settling
    def pca_project(self, X, mean, components):
        """``Y [N, d] = (X - mean) @ components.T`` for ``components`` ``[d, D]`` (``sit_pca_project``)."""
        X, mean, components = _f64(X), _f64(mean).reshape(-1), _f64(components)
        assert X.ndim == 2 and components.ndim == 2 and components.shape[1] == X.shape[1] == len(mean)
        N, D = X.shape
        d = components.shape[0]
        Y = np.zeros((N, d))
        self._check(self.lib.sit_pca_project(self._h, _d(X), N, D, _d(mean), _d(components), d, _d(Y)))
        return Y

    @_settling
    def dpc_graph(self, Y, fraction=0.02):
        """``(kernel_size, density [N], delta [N], neighbour int32 [N], info)`` (``sit_dpc_graph``): what ``pydpc.Cluster(Y,
        fraction)`` computes for the points ``Y`` ``[N, d]``, by the definitions of ``csrc/dpc_plan.h``.  ``info``: the kernel
        milliseconds and the number of pairs."""
        Y = _f64(Y)
        assert Y.ndim == 2
        N, d = Y.shape
        ks = C.c_double(0.0)
        density, delta, nbr, info = np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int32), np.zeros(2)
        self._check(self.lib.sit_dpc_graph(self._h, _d(Y), N, d, float(fraction), C.byref(ks), _d(density), _d(delta), _ptr(nbr),
                                           _d(info)))
        return ks.value, density, delta, nbr, {"kernel_ms": float(info[0]), "pairs": int(info[1])}

    @_settling
    def dpc_assign(self, density, delta, neighbour, min_density, min_delta, dvecs_to_site=None, K=0):
        """``(membership int32 [N], clusters int32 [n_clusters], votes int64 [K, n_clusters] or None)`` (``sit_dpc_assign``):
        centres are the points with ``density > min_density`` and ``delta > min_delta``, every other point follows its neighbour;
        ``votes[s, m]`` counts the points of site ``dvecs_to_site[i] == s`` with membership ``m``."""
        density, delta = _f64(density).reshape(-1), _f64(delta).reshape(-1)
        neighbour = _i32(neighbour).reshape(-1)
        N = len(density)
        assert len(delta) == N == len(neighbour)
        K = int(K) if dvecs_to_site is not None else 0
        site = _i64(dvecs_to_site).reshape(-1) if dvecs_to_site is not None else None
        assert site is None or len(site) == N
        membership, clusters = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
        nc = i64(0)
        guess = int(np.count_nonzero((density > min_density) & (delta > min_delta)))
        votes = np.zeros((K, guess), dtype=np.int64) if K > 0 else None
        self._check(self.lib.sit_dpc_assign(self._h, _d(density), _d(delta), _ptr(neighbour), N, float(min_density), float(min_delta),
                                            _i(site), K, _ptr(membership), _ptr(clusters), C.byref(nc), _i(votes),
                                            0 if votes is None else votes.size))
        assert int(nc.value) == guess
        return membership, clusters[:guess].copy(), votes

    # ---- RCCL exchange of the frame-sharded path (csrc/comm.hip) ----
    def comm_create(self, unique_id, rank, world):
        uid = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
        assert uid.size == 128
        self._check(self.lib.sit_comm_create(self._h, _ptr(uid), int(rank), int(world)))

    def comm_destroy(self):
        self.lib.sit_comm_destroy(self._h)

    def comm_info(self):
        """What the RCCL communicator reports about itself (``sit_comm_info``)."""
        v = np.zeros(6, dtype=np.int32)
        self._check(self.lib.sit_comm_info(self._h, _ptr(v)))
        return {"ranks": int(v[0]), "rank": int(v[1]), "device": int(v[2]), "rccl_version": int(v[3]),
                "asked_ranks": int(v[4]), "asked_rank": int(v[5])}

    def comm_allreduce(self, arr, op="sum"):
        """In place on a contiguous float64 / int64 / uint64 array."""
        code = {np.dtype(np.float64): 0, np.dtype(np.int64): 1, np.dtype(np.uint64): 2}[arr.dtype]
        self._check(self.lib.sit_comm_allreduce(self._h, _void(arr), arr.size, code, {"sum": 0, "min": 1, "max": 2}[op]))
        return arr

    def comm_allgather(self, send, world):
        send = np.ascontiguousarray(send)
        recv = np.empty((world,) + send.shape, dtype=send.dtype)
        self._check(self.lib.sit_comm_allgather(self._h, _void(send), _void(recv), send.nbytes))
        return recv

    def comm_broadcast(self, arr, root):
        self._check(self.lib.sit_comm_broadcast(self._h, _void(arr), arr.nbytes, int(root)))
        return arr

    def comm_barrier(self):
        self._check(self.lib.sit_comm_barrier(self._h))

    def comm_attach(self, comm_ctx):
        """``gram`` / ``weighted_row_sums`` (and their limbs) of this context return the sums over all ranks of
        ``comm_ctx``'s communicator, reduced on the device (``sit_comm_attach``); ``None`` detaches."""
        self._check(self.lib.sit_comm_attach(self._h, comm_ctx._h if comm_ctx is not None else None))

    def _timer_slots(self, n=24):
        """The first ``n`` slots of ``sit_timers``: three blocks of 8 - the last lap of every stage in ms, the sum of all
        its laps, their number; slots 0-6 of a block are ``_STAGES``, slot 7 the ``k_clamp`` launches."""
        t = np.zeros(n)
        self.lib.sit_timers(self._h, _d(t), n)
        return t

    def timers(self):
        return dict(zip(_STAGES, self._timer_slots(8)))

    def timer_totals(self):
        """(sum of all laps in ms, number of laps) per stage since the context was made."""
        t = self._timer_slots()
        return {k: (float(t[8 + i]), int(t[16 + i])) for i, k in enumerate(_STAGES)}

    def clamp_kernel_time(self):
        """(sum in ms, number) of the ``k_clamp`` launches of ``clamp_trajectory`` since the context was made: the
        kernel alone, without the copies of a call (slot 7 of ``sit_timers``)."""
        t = self._timer_slots()
        return float(t[15]), int(t[23])

    def info(self):
        v = np.zeros(29)
        self.lib.sit_info(self._h, _d(v), 29)
        keys = ["row_width", "mean_candidates_loose", "tight_width", "mean_candidates_tight", "delta",
                "fallback_frames"]
        out = dict(zip(keys, v[:6]))
        out["grid_loose"] = [int(x) for x in v[6:9]]
        out["grid_tight"] = [int(x) for x in v[9:12]]
        out["frames_per_workgroup"] = int(v[12])
        out["fit_batches"], out["fit_serial_rows"], out["fit_rewalks"] = int(v[13]), int(v[14]), int(v[15])
        out["fill_kernel"], out["survivors_per_wave"], out["waves_per_workgroup"] = int(v[16]), int(v[17]), int(v[18])
        out["fit_capacity_hit"], out["fit_stop_row"] = int(v[19]), int(v[20])
        out["task_table_per_wave"] = int(v[21])
        out["assignment_fused"] = bool(v[22])
        out["band_redos"] = int(v[23])
        out["census"] = [float(x) for x in v[24:28]]
        out["fill_slot_width"] = int(v[28])
        return out

    def candidate_table(self, which):
        """The pruning table as it lies on the device (``sit_candidate_table``; diagnostic): ``which`` 0 = the loose table of
        ``set_basis``, 1 = the tight table of the first ``fill``.  A dict of ``grid`` [3], ``displacement``, ``rb``, ``total``,
        ``off`` int32 [bins + 1], ``list`` int32 [total], ``crit`` uint8 [total].  ``ValueError`` when there is no such table."""
        G = np.zeros(3, dtype=np.int32)
        disp, rb, total = C.c_double(0), C.c_double(0), i64(0)
        head = (self._h, int(which), _ptr(G), C.byref(disp), C.byref(rb), C.byref(total))
        self._check(self.lib.sit_candidate_table(*head, 0, None, 0, None, None))
        nb, n = int(G[0]) * int(G[1]) * int(G[2]), int(total.value)
        off = np.zeros(nb + 1, dtype=np.int32)
        lst = np.zeros(max(n, 1), dtype=np.int32)
        crit = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.lib.sit_candidate_table(*head, nb + 1, _ptr(off), len(lst), _ptr(lst), _ptr(crit)))
        return {"grid": [int(x) for x in G], "displacement": disp.value, "rb": rb.value, "total": n, "off": off,
                "list": lst[:n], "crit": crit[:n]}

    def synchronize(self):
        self._check(self.lib.sit_synchronize(self._h))
