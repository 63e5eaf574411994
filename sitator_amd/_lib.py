"""ctypes binding of ``libsitator_hip.so`` (C-ABI declared in ``include/sitator_hip.h``).

There is no CPU fallback: if the library is missing, or a call fails, this module raises.
"""
import ctypes as C
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
_vp = C.c_void_p
i64 = C.c_int64


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
    "sit_gram_limbs": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _ip]),
    "sit_weighted_row_sums_limbs": (C.c_int, [_vp, C.c_int, i64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "sit_best_match": (C.c_int, [_vp, _dp, _ip, _dp, _dp]),
    "sit_best_match_groups": (C.c_int, [_vp, C.POINTER(C.c_int32), _dp, i64, _ip, _dp, _dp]),
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
    "sit_comm_allreduce": (C.c_int, [_vp, C.c_void_p, i64, C.c_int, C.c_int]),
    "sit_comm_allgather": (C.c_int, [_vp, C.c_void_p, C.c_void_p, i64]),
    "sit_comm_broadcast": (C.c_int, [_vp, C.c_void_p, i64, C.c_int]),
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


def comm_unique_id():
    """ncclGetUniqueId: 128 bytes that rank 0 makes and every rank of the job receives."""
    uid = np.zeros(128, dtype=np.uint8)
    if load().sit_comm_unique_id(uid.ctypes.data_as(_u8p)) != 0:
        raise RuntimeError("sit_comm_unique_id failed (librccl.so not loadable?)")
    return uid.tobytes()


def device_count():
    n = C.c_int(0)
    load().sit_device_count(C.byref(n))
    return n.value


def group_plan(n_entries, K):
    """``(entries per chunk, chunks, LDS form, largest K of the LDS form)`` of ``group_by_site`` (``sit_group_plan``)."""
    out = np.zeros(4, dtype=np.int64)
    if load().sit_group_plan(int(n_entries), int(K), _i(out)) != OK:
        raise ValueError("group_plan: beyond the capacity of group_by_site")
    return int(out[0]), int(out[1]), bool(out[2]), int(out[3])


def hull_plan():
    """``(facet capacity, open-edge capacity, threads per workgroup, LDS bytes per workgroup)`` of ``grouped_hull_volumes``
    (``sit_hull_plan``)."""
    out = np.zeros(4, dtype=np.int64)
    load().sit_hull_plan(_i(out))
    return tuple(int(v) for v in out)


def barrier_plan(cell, rc):
    """``{"translations": (n0, n1, n2), "tile": static atoms per LDS tile, "threads": per workgroup, "lds_bytes": per workgroup}``
    of ``barrier_energies`` for ``cell`` (rows are the cell vectors) and the cutoff ``rc`` (``sit_barrier_plan``)."""
    out = np.zeros(6, dtype=np.int64)
    cell = _f64(cell).reshape(3, 3)
    if load().sit_barrier_plan(_d(cell), float(rc), _i(out)) != OK:
        raise ValueError("barrier_plan: a degenerate cell, or rc not positive or beyond 255 perpendicular heights of the cell")
    return {"translations": tuple(int(v) for v in out[:3]), "tile": int(out[3]), "threads": int(out[4]), "lds_bytes": int(out[5])}


def soap_plan(cell, cutoff, n_species, n_max, l_max):
    """The plan of ``soap_vectors`` / ``soap_site_averages`` for ``cell`` (rows are the cell vectors) (``sit_soap_plan``): the
    translations, the workgroup, the neighbours staged at once, the LDS bytes, the limits and the lengths of a vector.  Beyond a
    limit: ``RuntimeError``."""
    out = np.zeros(12, dtype=np.int64)
    cell = _f64(cell).reshape(3, 3)
    rc = load().sit_soap_plan(_d(cell), float(cutoff), int(n_species), int(n_max), int(l_max), _i(out))
    limits = {"max_l": int(out[6]), "max_n": int(out[7]), "max_species": int(out[8])}
    if rc == E_CAPACITY:
        raise RuntimeError("soap_plan: l_max, n_max or the number of environment species is beyond %r" % limits)
    if rc != OK:
        raise ValueError("soap_plan: a degenerate cell, or a cutoff not positive or beyond 255 perpendicular heights of the cell")
    plan = {"translations": tuple(int(v) for v in out[:3]), "threads": int(out[3]), "nbr_cap": int(out[4]), "lds_bytes": int(out[5]),
            "n_coef": int(out[9]), "n_dim": int(out[10]), "n_dim_crossover": int(out[11])}
    plan.update(limits)
    return plan


def dpc_plan(d=1):
    """The plan of ``dpc_graph`` for points of ``d`` coordinates (``sit_dpc_plan``): the workgroup, the tile, the digits and passes
    of the radix select, the limits and the LDS bytes.  Beyond the largest ``d``: ``RuntimeError``."""
    out = np.zeros(12, dtype=np.int64)
    rc = load().sit_dpc_plan(int(d), _i(out))
    keys = ["threads", "tile", "digit_bits", "passes", "max_d", "lds_bytes", "segments", "max_n", "pca_rows", "pca_edge", "pca_max_d",
            "pca_max_n"]
    plan = {k: int(v) for k, v in zip(keys, out)}
    if rc == E_CAPACITY:
        raise RuntimeError("dpc_plan: more than %d coordinates per point" % plan["max_d"])
    if rc != OK:
        raise ValueError("dpc_plan: d must be at least 1")
    return plan


def voronoi_plan(cell, S):
    """The plan of ``voronoi_nodes`` for ``cell`` (rows are the cell vectors) and ``S`` atoms (``sit_voronoi_plan``): the caps, the
    workgroup, and the first search radius with its growth factor."""
    out, rad = np.zeros(8, dtype=np.int64), np.zeros(2)
    cell = _f64(cell).reshape(3, 3)
    if load().sit_voronoi_plan(_d(cell), int(S), _i(out), _d(rad)) != OK:
        raise ValueError("voronoi_plan: a degenerate cell or no atom")
    keys = ["neighbour_cap", "record_cap", "member_cap", "threads", "lds_bytes", "max_rounds", "record_bytes", "inverse_shape_min"]
    plan = {k: int(v) for k, v in zip(keys, out)}
    plan["first_radius"], plan["growth"] = float(rad[0]), float(rad[1])
    return plan


COORDENV_SHAPES = ("S:1", "L:2", "TL:3", "T:4", "S:4", "T:5", "S:5", "O:6", "T:6", "PB:7", "C:8", "SA:8")   # library order


def coordenv_plan():
    """The plan of ``coordination_environments`` (``sit_coordenv_plan``): the caps, the workgroup, and the shape library as
    ``"symbols"``, ``"shape_n"`` and ``"shapes"`` (a list of ``[n, 3]`` unit vertices)."""
    out, sn, co = np.zeros(8, dtype=np.int64), np.zeros(len(COORDENV_SHAPES), dtype=np.int32), np.zeros((len(COORDENV_SHAPES), 8, 3))
    if load().sit_coordenv_plan(_i(out), sn.ctypes.data_as(_i32p), _d(co)) != OK:
        raise ValueError("coordenv_plan")
    keys = ["neighbour_cap", "vertex_cap", "face_cap", "coordination_cap", "max_n", "threads", "lds_bytes", "n_shapes"]
    plan = {k: int(v) for k, v in zip(keys, out)}
    assert plan["n_shapes"] == len(COORDENV_SHAPES)
    plan["symbols"], plan["shape_n"] = list(COORDENV_SHAPES), [int(v) for v in sn]
    plan["shapes"] = [co[s, :sn[s]].copy() for s in range(len(COORDENV_SHAPES))]
    return plan


def release_cached_memory():
    """Returns the idle large device buffers the library keeps between contexts (sit_release_cached_memory)."""
    load().sit_release_cached_memory()


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


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
        if rc == E_INVALID:
            raise ValueError(self.message())
        if rc == E_NOT_CONVERGED:
            raise ValueError(self.message())
        if rc in (E_HIP, E_CAPACITY):
            raise RuntimeError("libsitator_hip: %s" % self.message())
        raise errors.DeviceDomainError(rc, err.frame if err else -1, err.index if err else -1)

    # -- PBCCalculator surface
    def wrap_points(self, pts):
        pts = _f64(pts)
        assert pts.ndim == 2 and pts.shape[1] == 3, "Points must be 3D"
        self._check(self.lib.sit_wrap_points(self._h, _d(pts), len(pts)))
        return pts

    def distances(self, pt1, pts2):
        pt1 = _f64(pt1)
        pts2 = _f64(pts2)
        out = np.empty(len(pts2))
        self._check(self.lib.sit_distances(self._h, _d(pt1), _d(pts2), len(pts2), _d(out)))
        return out

    def average(self, pts, weights=None):
        pts = _f64(pts)
        w = None if weights is None else _f64(weights)
        out = np.empty(3)
        self._check(self.lib.sit_average(self._h, _d(pts), None if w is None else _d(w), len(pts), _d(out)))
        return out

    def min_image(self, ref, pts):
        """``(moved points [n, 3], codes int32 [n])``: every ``pts[p]`` moved to its periodic image nearest ``ref[p]`` and
        the reference's code ``100 i + 10 j + k`` of that image (``sit_min_image``)."""
        ref = _f64(ref).reshape(-1, 3)
        pts = np.array(pts, dtype=np.float64).reshape(-1, 3)
        assert ref.shape == pts.shape
        code = np.zeros(len(pts), dtype=np.int32)
        self._check(self.lib.sit_min_image(self._h, _d(ref), _d(pts), len(pts), code.ctypes.data_as(_i32p)))
        return pts, code

    def site_vertex_distances(self, centers, ref_static, verts):
        centers = _f64(centers); ref_static = _f64(ref_static); verts = _i64(verts)
        out = np.empty(verts.shape)
        self._check(self.lib.sit_site_vertex_distances(self._h, _d(centers), _d(ref_static), _i(verts), verts.shape[0],
                                                       verts.shape[1], len(ref_static), _d(out)))
        return out

    # -- residency
    def set_basis(self, ref_static, verts, vert_dists, midpoint, steepness, static_threshold):
        ref_static = _f64(ref_static)
        verts = _i64(verts)
        vert_dists = _f64(vert_dists)
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

    def set_frames(self, frames, static_idx, mobile_idx, frame0=0):
        frames = _f64(frames)
        static_idx = _i64(static_idx)
        mobile_idx = _i64(mobile_idx)
        self.F, self.A = frames.shape[0], frames.shape[1]
        self.M = len(mobile_idx)
        self.N = self.F * self.M
        self.frame0 = int(frame0)
        self._check(self.lib.sit_set_frames(self._h, _d(frames), self.F, self.A, _i(static_idx), len(static_idx),
                                            _i(mobile_idx), self.M, self.frame0))

    def upload_fill_fit(self, frames, static_idx, mobile_idx, frame0, dynamic_lattice_mapping, relaxed_lattice_checks,
                        check_for_zeros, fit_threshold):
        """``set_frames`` + ``fill`` + the first pass of ``fit_centers`` with the upload overlapped
        (``sit_upload_fill_fit``).  Returns ``(rc, n_all_zero, err, fitted)``."""
        frames = _f64(frames)
        static_idx = _i64(static_idx)
        mobile_idx = _i64(mobile_idx)
        self.F, self.A = frames.shape[0], frames.shape[1]
        self.M = len(mobile_idx)
        self.N = self.F * self.M
        self.frame0 = int(frame0)
        p = FillParams.make(dynamic_lattice_mapping, relaxed_lattice_checks, check_for_zeros, 1, 0, 1, 0.0)
        nz = i64(0)
        err = SitError()
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
        nz = i64(0)
        err = SitError()
        if assign:
            self.labels_version += 1
            self.labels_digest = None
        self._last_fill = p
        rc = self.lib.sit_fill(self._h, C.byref(p), C.byref(nz), C.byref(err))
        self._deferred = self._deferred + 1 if (defer and rc == OK) else 0
        return rc, nz.value, err

    def fill_result(self):
        """Status, ``n_all_zero`` and error of the deferred passes in flight (waits for them; the first failure wins).
        A pass whose rows outgrew the buffers measured on the leading frames (``SIT_RETRY``) is run again, blocking."""
        nz = i64(0)
        err = SitError()
        rc = self.lib.sit_fill_result(self._h, C.byref(nz), C.byref(err))
        self._deferred = 0
        if rc == RETRY:
            p = self._last_fill
            p.defer = 0
            rc = self.lib.sit_fill(self._h, C.byref(p), C.byref(nz), C.byref(err))
        return rc, nz.value, err

    def static_seen(self, local_frame):
        seen = np.zeros(self.S, dtype=np.uint8)
        self._check(self.lib.sit_static_seen(self._h, int(local_frame), seen.ctypes.data_as(_u8p)))
        return seen

    def rows_dense(self, row0=0, nrows=None):
        nrows = self.N - row0 if nrows is None else nrows
        out = np.empty((nrows, self.D))
        self._check(self.lib.sit_get_rows_dense(self._h, int(row0), int(nrows), _d(out)))
        return out

    def rows_sparse(self, row0=0, nrows=None):
        nrows = self.N - row0 if nrows is None else nrows
        W = self.row_width()
        nnz = np.empty(nrows, dtype=np.int32)
        idx = np.empty((W, nrows), dtype=np.int32)
        val = np.empty((W, nrows))
        self._check(self.lib.sit_get_rows_sparse(self._h, int(row0), int(nrows), nnz.ctypes.data_as(_i32p),
                                                 idx.ctypes.data_as(_i32p), _d(val)))
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

    def fit_push_stored_rows(self, threshold):
        self._check(self.lib.sit_fit_push_stored_rows(self._h, float(threshold)))

    def fit_push_dense_rows(self, rows, weights, threshold):
        rows = _f64(rows).reshape(-1, self.D)
        weights = _i64(weights)
        self._check(self.lib.sit_fit_push_dense_rows(self._h, _d(rows), _i(weights), len(rows), float(threshold)))

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

    def predict(self, threshold, fetch=True):
        self.labels_version += 1
        self.labels_digest = None
        counts = np.zeros(self.K, dtype=np.int64)
        if fetch:
            labels, confs = self._assignment_arrays()
            self._check(self.lib.sit_predict(self._h, float(threshold), _i(labels), _d(confs), _i(counts)))
            return labels, confs, counts
        self._check(self.lib.sit_predict(self._h, float(threshold), None, None, _i(counts)))
        return None, None, counts

    def assignments(self):
        labels = np.empty(self.N, dtype=np.int64)
        confs = np.empty(self.N)
        counts = np.zeros(self.K, dtype=np.int64)
        self._check(self.lib.sit_get_assignments(self._h, _i(labels), _d(confs), _i(counts)))
        return labels, confs, counts

    def count_zero_rows(self):
        """(number of all-zero rows, index of the first one or -1)."""
        n, first = i64(0), i64(0)
        self._check(self.lib.sit_count_zero_rows(self._h, C.byref(n), C.byref(first)))
        return n.value, first.value

    # -- mcl support
    def gram(self):
        G = np.empty((self.D, self.D))
        seen = np.empty(self.D, dtype=np.int64)
        self._check(self.lib.sit_gram(self._h, _d(G), _i(seen)))
        return G, seen

    def gram_limbs(self):
        """The Gram matrix as exact integers (hi, lo) in units of 2^-80 (see ``exact_sum_across``), and ``seen``."""
        hi = np.empty((self.D, self.D), dtype=np.uint64)
        lo = np.empty((self.D, self.D), dtype=np.uint64)
        seen = np.empty(self.D, dtype=np.int64)
        u64p = C.POINTER(C.c_uint64)
        self._check(self.lib.sit_gram_limbs(self._h, hi.ctypes.data_as(u64p), lo.ctypes.data_as(u64p), _i(seen)))
        return hi, lo, seen

    def weighted_row_sums_limbs(self, K, weighted=True):
        n = K * self.D + K
        hi = np.empty(n, dtype=np.uint64)
        lo = np.empty(n, dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._check(self.lib.sit_weighted_row_sums_limbs(self._h, int(weighted), int(K), hi.ctypes.data_as(u64p),
                                                         lo.ctypes.data_as(u64p)))
        return hi, lo

    def best_match(self, c):
        c = _f64(c)
        row = i64(0)
        dot = C.c_double(0)
        nrm = C.c_double(0)
        self._check(self.lib.sit_best_match(self._h, _d(c), C.byref(row), C.byref(dot), C.byref(nrm)))
        return row.value, dot.value, nrm.value

    def best_match_groups(self, group_of_dim, cvec, G):
        """``best_match`` for ``G`` centres with disjoint supports in one pass: (rows, dots, norms), each ``[G]``."""
        grp = np.ascontiguousarray(group_of_dim, dtype=np.int32)
        cvec = _f64(cvec)
        assert grp.shape == (self.D,) and cvec.shape == (self.D,)
        rows = np.empty(G, dtype=np.int64)
        dots = np.empty(G)
        nrms = np.empty(G)
        self._check(self.lib.sit_best_match_groups(self._h, grp.ctypes.data_as(C.POINTER(C.c_int32)), _d(cvec), G,
                                                   _i(rows), _d(dots), _d(nrms)))
        return rows, dots, nrms

    def weighted_row_sums(self, K, weighted=True):
        sums = np.empty((K, self.D))
        wsum = np.empty(K)
        self._check(self.lib.sit_weighted_row_sums(self._h, int(weighted), int(K), _d(sums), _d(wsum)))
        return sums, wsum

    # -- site centres / occupancy
    def site_anchors(self, K, weighted):
        wmax = np.empty(K)
        first = np.empty(K, dtype=np.int64)
        pts = np.empty((K, 3))
        self._check(self.lib.sit_site_anchors(self._h, int(weighted), int(K), _d(wmax), _i(first), _d(pts)))
        return wmax, first, pts

    def site_sums(self, K, weighted, anchors):
        anchors = _f64(anchors)
        sums = np.empty((K, 4))
        self._check(self.lib.sit_site_sums(self._h, int(weighted), int(K), _d(anchors), _d(sums)))
        return sums

    def check_occupancy(self, K, max_per_site):
        a, b, c = i64(0), i64(0), i64(0)
        err = SitError()
        rc = self.lib.sit_check_occupancy(self._h, int(K), int(max_per_site), C.byref(a), C.byref(b), C.byref(c),
                                          C.byref(err))
        return rc, a.value, b.value, c.value, err

    def set_assignments(self, labels, confs=None, frame0=0):
        self.labels_version += 1
        self.labels_digest = None
        labels = _i64(labels)
        F, M = labels.shape
        c = None if confs is None else _f64(confs)
        self._check(self.lib.sit_set_assignments(self._h, _i(labels), None if c is None else _d(c), F, M, int(frame0)))
        self.F, self.M, self.N, self.frame0 = F, M, F * M, int(frame0)

    def site_counts(self, K):
        counts = np.zeros(int(K), dtype=np.int64)
        self._check(self.lib.sit_site_counts(self._h, int(K), _i(counts)))
        return counts

    def cooccupancy(self, K):
        """``bool[K, K]``: entry (a, b) says whether some resident frame has one ion on site a and one on site b
        (``sit_cooccupancy``; at most 16384 sites)."""
        K = int(K)
        co = np.zeros((K, K), dtype=np.uint8)
        rc = self.lib.sit_cooccupancy(self._h, K, co.ctypes.data_as(_u8p))
        # a label beyond the sites: the reference's connmat[site, frame] raises this (MergeSitesByThreshold.py:70)
        self._check_index(rc)
        return co.view(np.bool_)

    JUMP_NONE = -(1 << 63)

    def jump_sources(self, unknown_as_jump=False, last_known_in=None):
        src = np.empty((self.F, self.M), dtype=np.int64)
        last_out = np.empty(self.M, dtype=np.int64)
        lin = None if last_known_in is None else _i64(last_known_in)
        self._check(self.lib.sit_jump_sources(self._h, int(unknown_as_jump), None if lin is None else _i(lin),
                                              _i(src), _i(last_out)))
        return src, last_out

    def jump_list(self, unknown_as_jump=False, last_known_in=None):
        """Jumps as an ``[n, 4]`` array of (frame, mobile atom, from site, to site), frame-major, and the last known
        site of every ion after this context's frames."""
        last_out = np.empty(self.M, dtype=np.int64)
        lin = None if last_known_in is None else _i64(last_known_in)
        cap = 1 << 16
        while True:
            rec = np.empty((cap, 4), dtype=np.int64)
            n = i64(0)
            self._check(self.lib.sit_jump_list(self._h, int(unknown_as_jump), None if lin is None else _i(lin), cap,
                                               _i(rec), C.byref(n), _i(last_out)))
            if n.value <= cap:
                break
            cap = int(n.value)
        rec = rec[:n.value]
        order = np.lexsort((rec[:, 1], rec[:, 0]))
        return rec[order], last_out

    def jump_analysis(self, K, last_known_in=None, time_at_current_in=None):
        n_ij = np.empty((K, K)); tsum = np.empty((K, K)); tn = np.empty((K, K), dtype=np.int64)
        total = np.empty(K, dtype=np.int64); nprob = i64(0)
        lout = np.empty(self.M, dtype=np.int64); tout = np.empty(self.M, dtype=np.int64)
        lin = None if last_known_in is None else _i64(last_known_in)
        tin = None if time_at_current_in is None else _i64(time_at_current_in)
        rc = self.lib.sit_jump_analysis(self._h, int(K), None if lin is None else _i(lin),
                                        None if tin is None else _i(tin), _d(n_ij), _d(tsum), _i(tn), _i(total),
                                        C.byref(nprob), _i(lout), _i(tout))
        # a label beyond the site tables: the reference's fancy indexing raises this (dynamics/JumpAnalysis.py:75-88)
        self._check_index(rc)
        return n_ij, tsum, tn, total, nprob.value, lout, tout

    def assign_last_known(self, frame_threshold, last_known_in=None, time_unknown_in=None, out=None):
        """``out``: a C-contiguous int64 [F, M] array that receives the new labels (else a fresh one)."""
        labels = np.empty((self.F, self.M), dtype=np.int64) if out is None else out
        assert labels.dtype == np.int64 and labels.flags.c_contiguous and labels.shape == (self.F, self.M)
        self.labels_version += 1            # the kernel rewrites the resident labels in place
        self.labels_digest = None
        fmax = np.zeros(max(self.F, 1), dtype=np.int32)
        st = np.zeros(3, dtype=np.int64)
        lout = np.empty(self.M, dtype=np.int64); tout = np.empty(self.M, dtype=np.int64)
        lin = None if last_known_in is None else _i64(last_known_in)
        tin = None if time_unknown_in is None else _i64(time_unknown_in)
        self._check(self.lib.sit_assign_last_known(self._h, int(frame_threshold), None if lin is None else _i(lin),
                                                   None if tin is None else _i(tin), _i(labels),
                                                   fmax.ctypes.data_as(_i32p), _i(st), _i(lout), _i(tout)))
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

    def label_ends(self):
        """Per ion the first and the last label != -1 of this context's frames (``ENDS_NONE`` where it has none)."""
        first = np.full(self.M, self.ENDS_NONE, dtype=np.int64)
        last = np.full(self.M, self.ENDS_NONE, dtype=np.int64)
        self._check(self.lib.sit_label_ends(self._h, _i(first), _i(last)))
        return first, last

    def replace_unassigned(self, mode, before_in=None, after_in=None):
        """The labels with every -1 replaced by the nearest known label before it (``mode`` 0) or after it (1);
        ``before_in`` / ``after_in`` ([M]): what holds before the first and after the last frame (default -1)."""
        b, a = self._halo_pair(before_in, after_in)
        out = np.empty((self.F, self.M), dtype=np.int64)
        self._check(self.lib.sit_replace_unassigned(self._h, int(mode), None if b is None else _i(b),
                                                    None if a is None else _i(a), _i(out)))
        return out

    def unknown_runs(self, before_in=None, after_in=None):
        """``(records, n_positions)``: every maximal run of -1 as (ion, start, end, before, after, pos_offset), ion-major
        and by start; start / end are global frame numbers (``sit_unknown_runs``)."""
        b, a = self._halo_pair(before_in, after_in)
        cap = 1 << 16
        while True:
            rec = np.empty((cap, 6), dtype=np.int64)
            n, npos = i64(0), i64(0)
            self._check(self.lib.sit_unknown_runs(self._h, None if b is None else _i(b), None if a is None else _i(a),
                                                  cap, _i(rec), C.byref(n), C.byref(npos)))
            if n.value <= cap:
                break
            cap = int(n.value)
        return rec[:n.value], int(npos.value)

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

    def running_mode(self, wleft, wright, threshold, replace_unknown, n_sites=0):
        """The smoothed labels, and (``n_sites`` > 0) how often every site occurs among them."""
        out = np.empty((self.F, self.M), dtype=np.int64)
        counts = np.zeros(int(n_sites), dtype=np.int64) if n_sites > 0 else None
        self._check(self.lib.sit_running_mode(self._h, int(wleft), int(wright), int(threshold), int(replace_unknown), _i(out),
                                              int(n_sites), None if counts is None else _i(counts)))
        return (out, counts) if counts is not None else out

    def recenter(self, arr, masses, factors, add3=None):
        assert arr.dtype == np.float64 and arr.flags.c_contiguous and arr.ndim == 3 and arr.shape[2] == 3
        masses = _f64(masses); factors = _f64(factors)
        a3 = None if add3 is None else _f64(add3)
        self._check(self.lib.sit_recenter(self._h, _d(arr), arr.shape[0], arr.shape[1], _d(masses), _d(factors),
                                          None if a3 is None else _d(a3)))

    def recenter_resident(self, masses, factors, add3=None):
        """Recentre the frames resident after ``set_frames`` in place on the device (``sit_recenter_resident``)."""
        masses = _f64(masses); factors = _f64(factors)
        assert len(masses) == self.A and len(factors) == self.A
        a3 = None if add3 is None else _f64(add3)
        self._check(self.lib.sit_recenter_resident(self._h, _d(masses), _d(factors), None if a3 is None else _d(a3)))

    def _selection(self, positions, atoms):
        """``(positions, idx, F, n_sel)``: a host ``[F, n_sel, 3]`` array, or ``atoms`` as columns of the resident frames."""
        if positions is not None:
            positions = _f64(positions)
            assert positions.ndim == 3 and positions.shape[2] == 3
            return positions, None, positions.shape[0], positions.shape[1]
        idx = _i64(atoms).reshape(-1)
        return None, idx, self.F, len(idx)

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
        avg = np.empty(n_sel)
        power = np.empty(n_sel)
        spec = np.empty((n_sel, nbins), dtype=np.complex128) if spectrum else None
        spd = np.empty((n_sel, max(F - 1, 0))) if speeds else None
        self._check(self.lib.sit_speed_spectrum(
            self._h, None if positions is None else _d(positions), int(F), None if idx is None else _i(idx), int(n_sel),
            _d(freqs), fmask.ctypes.data_as(_u8p), int(workspace_bytes), _d(avg), _d(power),
            None if spec is None else spec.ctypes.data_as(_dp), None if spd is None else _d(spd)))
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
        rc = self.lib.sit_msd(
            self._h, None if positions is None else _d(positions), int(F), None if idx is None else _i(idx), int(n_sel),
            int(bool(unwrap)), int(max_lag), None if lag_arr is None else _i(lag_arr), int(n_lags), int(bool(collective)),
            int(workspace_bytes), _d(out), None if out4 is None else _d(out4), None if coll is None else _d(coll),
            None if img is None else img.ctypes.data_as(_i32p), C.byref(res))
        self._check(rc)
        return out, out4, coll, img, res.value

    # -- GenerateClampedTrajectory: reads labels and frames only (labels_version, rows and labels stay)
    def clamp_trajectory(self, role, fixed_pos, centers, wrap, pass_through_unassigned, positions=None, workspace_bytes=0):
        """``float64[F, A, 3]`` (``sit_clamp_trajectory``): per atom, by ``role[a]``, its real position (-1),
        ``fixed_pos[a]`` (-2) or the centre of the site that column ``role[a]`` of the resident labels names - as given
        with ``wrap``, else its periodic image nearest the atom's real position.  ``positions``: a host ``[F, A, 3]``
        float64 array; without it the frames resident after ``set_frames`` are read (none are needed with ``wrap``, no
        role -1 and no pass-through).  ``workspace_bytes``: cap on the device buffers of a chunk of frames (0: the default
        of 1 GiB).  An unassigned label without ``pass_through_unassigned`` raises ``errors.UnassignedClampError`` (a
        ``RuntimeError``; ``.first_unassigned`` = the smallest frame * M + column), a label ``>= len(centers)``
        ``IndexError``, any other argument that does not fit the context ``ValueError``."""
        role = np.ascontiguousarray(role, dtype=np.int32).reshape(-1)
        A = len(role)
        fixed_pos = _f64(fixed_pos).reshape(A, 3)
        centers = _f64(centers).reshape(-1, 3)
        if positions is not None:
            positions = _f64(positions)
            assert positions.ndim == 3 and positions.shape[1:] == (A, 3)
            F = positions.shape[0]
        else:
            F = self.F
        out = np.empty((F, A, 3))
        first = i64(-1)
        rc = self.lib.sit_clamp_trajectory(
            self._h, None if positions is None else _d(positions), int(F), int(A), role.ctypes.data_as(_i32p), _d(fixed_pos),
            _d(centers), len(centers), int(bool(wrap)), int(bool(pass_through_unassigned)), int(workspace_bytes), _d(out),
            C.byref(first))
        if rc == E_UNASSIGNED:
            raise errors.UnassignedClampError(first.value)
        # a label beyond the sites: the reference's centers_c[at_site] reads past the table (GenerateClampedTrajectory.pyx:99)
        self._check_index(rc)
        return out

    # -- per-site point clouds: reads labels and frames only (labels_version, rows and labels stay)
    def _check_index(self, rc):
        if rc == E_INVALID and self.message().startswith("index "):
            raise IndexError(self.message())
        self._check(rc)

    def group_by_site(self, K, positions=None, mobile_idx=None, workspace_bytes=0):
        """``offsets`` int64 ``[K + 1]`` of a stable grouping of the assigned entries ``frame * M + column`` of the resident
        labels by site (``sit_group_by_site``): sites ascending, entries ascending inside a site - the order of
        ``real_traj[:, mobile_mask][traj == site]``.  ``positions``: a host ``[F, A, 3]`` float64 array with ``mobile_idx``
        ``[M]`` naming the atoms of the label columns; without it the frames resident after ``set_frames`` are read.  The
        grouping stays on the device (``grouped_fetch``, ``grouped_bucket_averages``, ``grouped_recenter_step``) until the
        labels are rewritten.  A label ``>= K`` raises ``IndexError``, anything else that does not fit ``ValueError``."""
        K = int(K)
        offsets = np.zeros(K + 1, dtype=np.int64)
        if positions is not None:
            positions = _f64(positions)
            assert positions.ndim == 3 and positions.shape[2] == 3
            midx = _i64(mobile_idx).reshape(-1)
            F, A, M = positions.shape[0], positions.shape[1], len(midx)
        else:
            midx = None
            F, A, M = self.F, self.A, self.M
        rc = self.lib.sit_group_by_site(self._h, None if positions is None else _d(positions), int(F), int(A),
                                        None if midx is None else _i(midx), int(M), K, int(workspace_bytes), _i(offsets))
        self._check_index(rc)
        return offsets

    def grouped_fetch(self, first, n, points=True, confidences=False, entries=False):
        """``(points [n, 3], confidences [n], entries [n])`` of the elements ``[first, first + n)`` of the grouping, ``None``
        for what was not asked for.  ``ValueError`` ("stale ...") once the labels have been rewritten."""
        n = int(n)
        pts = np.empty((n, 3)) if points else None
        cf = np.empty(n) if confidences else None
        en = np.empty(n, dtype=np.int64) if entries else None
        self._check(self.lib.sit_grouped_fetch(self._h, int(first), n, None if pts is None else _d(pts),
                                               None if cf is None else _d(cf), None if en is None else _i(en)))
        return pts, cf, en

    def grouped_bucket_averages(self, K, n_avg, weighted):
        """``(centers [K, n_avg, 3], anchors [K, n_avg])``: ``PBCCalculator.average`` of the elements of every site at ranks
        ``i, i + n_avg, ...`` (``sit_grouped_bucket_averages``); NaN / -1 for sites of at most ``n_avg`` elements."""
        out = np.empty((int(K), int(n_avg), 3))
        anchors = np.empty((int(K), int(n_avg)), dtype=np.int64)
        self._check(self.lib.sit_grouped_bucket_averages(self._h, int(n_avg), int(bool(weighted)), _d(out), _i(anchors)))
        return out, anchors

    def grouped_recenter_step(self, i, n_recenterings, out):
        """Step ``i`` of the cumulative recentring of every site's points (``sit_grouped_recenter_step``) into ``out``
        ``[N, 3]`` (float64, C-contiguous; ``None``: not copied back).  An empty site raises ``IndexError``."""
        if out is not None:
            assert out.dtype == np.float64 and out.flags.c_contiguous and out.ndim == 2 and out.shape[1] == 3
        self._check_index(self.lib.sit_grouped_recenter_step(self._h, int(i), int(n_recenterings), None if out is None else _d(out)))
        return out

    def grouped_hull_volumes(self, K, vertex_mask=False):
        """``(volumes [K], status int32 [K], n_facets int32 [K], vertex_mask uint8 [N] or None)``: the convex hull of every
        site's points in the working copy as the last ``grouped_recenter_step`` left it (``sit_grouped_hull_volumes``).
        ``status`` 0: closed, the volume is the hull's; 1: fewer than 4 points; 2: an uncertain orientation test; 3: beyond
        the capacity of ``hull_plan()``; 4: not closed - the volume is NaN for all of these.  ``ValueError`` before step 0
        and for a stale grouping."""
        info = self.group_info()
        if int(K) != info["n_sites"]:
            raise ValueError("grouped_hull_volumes: K is not the number of sites of the grouping")
        vols = np.empty(int(K))
        status = np.empty(int(K), dtype=np.int32)
        nf = np.empty(int(K), dtype=np.int32)
        mask = np.zeros(info["n_grouped"], dtype=np.uint8) if vertex_mask else None
        self._check(self.lib.sit_grouped_hull_volumes(self._h, _d(vols), status.ctypes.data_as(_i32p), nf.ctypes.data_as(_i32p),
                                                      None if mask is None else mask.ctypes.data_as(_u8p)))
        return vols, status, nf, mask

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
        self._check(self.lib.sit_pathway_components(self._h, K, conn.ctypes.data_as(_u8p), _d(centers), int(n_images),
                                                    None if code is None else code.ctypes.data_as(_i32p),
                                                    root.ctypes.data_as(_i32p), C.byref(rounds)))
        return root, int(rounds.value), code

    # -- MergeSitesByBarrier: reads nothing of the context but its cell
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
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        coeffs = _f64(coeffs).reshape(-1)
        P, n = len(pairs), len(coeffs)
        en = np.empty((P, n)) if energies else None
        verdict = np.zeros((P, 3), dtype=np.uint8)
        code = np.zeros(P, dtype=np.int32) if codes else None
        self._check(self.lib.sit_barrier_energies(
            self._h, _d(static_pos), _d(eps), _d(sigma), len(static_pos), float(rc), _d(centers), len(centers),
            pairs.ctypes.data_as(_i32p), P, _d(coeffs), n, float(threshold), None if en is None else _d(en),
            verdict.ctypes.data_as(_u8p), None if code is None else code.ctypes.data_as(_i32p)))
        return en, verdict, code

    # -- VoronoiSiteGenerator: reads nothing of the context but its cell
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
        tail = (status.ctypes.data_as(_i32p), nbr.ctypes.data_as(_i32p), _d(info))
        self._check(self.lib.sit_voronoi_nodes(*head, 0, 0, C.byref(nn), C.byref(ni), None, None, None, None, *tail))
        n, m = int(nn.value), int(ni.value)
        centers, radii = np.zeros((n, 3)), np.zeros(n)
        offsets, indices = np.zeros(n + 1, dtype=np.int64), np.zeros(max(m, 1), dtype=np.int32)
        self._check(self.lib.sit_voronoi_nodes(*head, n, m, C.byref(nn), C.byref(ni), _d(centers), _d(radii), _i(offsets),
                                               indices.ctypes.data_as(_i32p), *tail))
        assert int(nn.value) == n and int(ni.value) == m
        keys = ["rounds", "final_radius", "max_neighbours", "records", "kernel_ms", "first_radius", "merge_status"]
        out_info = {k: (float(v) if k in ("final_radius", "kernel_ms", "first_radius") else int(v)) for k, v in zip(keys, info)}
        return {"centers": centers, "radii": radii, "vertices": [indices[offsets[j]:offsets[j + 1]].copy() for j in range(n)],
                "status": status, "nbr_count": nbr, "info": out_info}

    # -- SiteCoordinationEnvironment: reads nothing of the context but its cell
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
        per = (status.ctypes.data_as(_i32p), flags.ctypes.data_as(_i32p), n.ctypes.data_as(_i32p))
        tail = (shape.ctypes.data_as(_i32p), _d(best), _d(call), _d(conf), _d(info))
        self._check(self.lib.sit_coordination_environments(*head, 0, C.byref(ni), *per, None, None, None, None, *tail))
        computed = int(info[7])
        m = int(ni.value)
        offsets, indices = np.zeros(K + 1, dtype=np.int64), np.zeros(max(m, 1), dtype=np.int32)
        nd, na = np.zeros(max(m, 1)), np.zeros(max(m, 1))
        self._check(self.lib.sit_coordination_environments(*head, m, C.byref(ni), *per, _i(offsets), indices.ctypes.data_as(_i32p), _d(nd),
                                                           _d(na), *tail))
        assert int(ni.value) == m
        keys = ["rounds", "final_radius", "max_neighbours", "max_n", "cell_ms", "csm_ms", "first_radius", "fill_computed"]
        out_info = {k: (int(v) if k in ("rounds", "max_neighbours", "max_n", "fill_computed") else float(v)) for k, v in zip(keys, info)}
        out_info["size_computed"] = computed
        cut = lambda a: [a[offsets[j]:offsets[j + 1]].copy() for j in range(K)]
        return {"status": status[:K], "flags": flags[:K], "n": n[:K], "shape": shape[:K], "vertices": cut(indices), "norm_distance": cut(nd),
                "norm_angle": cut(na), "csm_best": best[:K], "csm_all": call[:K], "confidence": conf[:K], "info": out_info}

    # -- SOAP descriptors: soap_vectors reads nothing of the context but its cell, soap_site_averages labels and frames only
    def _soap_args(self, soap):
        """The tail of scalars and tables the SOAP entry points share, from a ``soap`` dict (``site_descriptors.soap_tables``), and
        the arrays its pointers point into (the caller holds them for the duration of the call)."""
        alpha, beta = _f64(soap["alpha"]), _f64(soap["beta"])
        L, n = int(soap["l_max"]) + 1, int(soap["n_max"])
        assert alpha.shape == (L, n) and beta.shape == (L, n, n)
        return (float(soap["cutoff"]), float(soap["cutoff_transition_width"]), float(soap["atom_sigma"]), int(soap["n_species"]), n,
                L - 1, int(bool(soap["crossover"])), _d(alpha), _d(beta), int(soap["n_dim"])), (alpha, beta)

    def soap_vectors(self, static_pos, species_idx, centers, soap, nbr_count=False):
        """``(out [P, n_dim], nbr_count int32 [P] or None)`` (``sit_soap_vectors``): the SOAP power spectrum of every centre among
        the atoms ``static_pos`` ``[S, 3]`` and all their periodic images under the context's cell; ``species_idx`` ``[S]``: the
        index of an atom's species in the environment list, -1 for an atom outside it.  ``soap``: the dict of
        ``site_descriptors.soap_tables``.  Beyond a capacity ``RuntimeError``, anything else that does not fit ``ValueError``."""
        static_pos = _f64(static_pos).reshape(-1, 3)
        species_idx = np.ascontiguousarray(species_idx, dtype=np.int32).reshape(-1)
        assert len(species_idx) == len(static_pos)
        centers = _f64(centers).reshape(-1, 3)
        tail, keep = self._soap_args(soap)
        P = len(centers)
        out = np.zeros((P, int(soap["n_dim"])))
        cnt = np.zeros(P, dtype=np.int32) if nbr_count else None
        self._check(self.lib.sit_soap_vectors(self._h, _d(static_pos), species_idx.ctypes.data_as(_i32p), len(static_pos), _d(centers), P,
                                              *tail, _d(out), None if cnt is None else cnt.ctypes.data_as(_i32p)))
        return out, cnt

    def soap_site_averages(self, K, static_idx, species_idx, mobile_idx, soap, stepsize=1, averaging=None, avg_descriptors_per_site=None,
                           positions=None, workspace_bytes=0):
        """``(descs [R, n_dim], counts [K], nr_of_descs [K], info)`` (``sit_soap_site_averages``, size call then fill call): the
        averaged SOAP vectors of ``SOAPDescriptorAverages`` on the resident labels; ``positions``: a host ``[F, A, 3]`` float64
        array, without it the frames resident after ``set_frames`` are read.  A label ``>= K`` raises ``IndexError``."""
        static_idx, mobile_idx = _i64(static_idx).reshape(-1), _i64(mobile_idx).reshape(-1)
        species_idx = np.ascontiguousarray(species_idx, dtype=np.int32).reshape(-1)
        assert len(species_idx) == len(static_idx)
        if positions is not None:
            positions = _f64(positions)
            assert positions.ndim == 3 and positions.shape[2] == 3
            F, A = positions.shape[0], positions.shape[1]
        else:
            F, A = self.F, self.A
        K = int(K)
        tail, keep = self._soap_args(soap)
        counts, nr = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        info = np.zeros(4)
        n_rows = i64(0)
        head = (self._h, None if positions is None else _d(positions), int(F), int(A), _i(static_idx), species_idx.ctypes.data_as(_i32p),
                len(static_idx), _i(mobile_idx), len(mobile_idx), K, int(stepsize), int(averaging or 0), int(avg_descriptors_per_site or 0))
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
    def pca_covariance(self, X):
        """``(mean [D], cov [D, D])`` of the rows ``X`` ``[N, D]`` (``sit_pca_covariance``): ``cov`` has the divisor
        ``max(N - 1, 1)``.  Beyond a capacity ``RuntimeError``, anything else that does not fit ``ValueError``."""
        X = _f64(X)
        assert X.ndim == 2
        N, D = X.shape
        mean, cov = np.zeros(D), np.zeros((D, D))
        self._check(self.lib.sit_pca_covariance(self._h, _d(X), N, D, _d(mean), _d(cov)))
        return mean, cov

    def pca_project(self, X, mean, components):
        """``Y [N, d] = (X - mean) @ components.T`` for ``components`` ``[d, D]`` (``sit_pca_project``)."""
        X, mean, components = _f64(X), _f64(mean).reshape(-1), _f64(components)
        assert X.ndim == 2 and components.ndim == 2 and components.shape[1] == X.shape[1] == len(mean)
        N, D = X.shape
        d = components.shape[0]
        Y = np.zeros((N, d))
        self._check(self.lib.sit_pca_project(self._h, _d(X), N, D, _d(mean), _d(components), d, _d(Y)))
        return Y

    def dpc_graph(self, Y, fraction=0.02):
        """``(kernel_size, density [N], delta [N], neighbour int32 [N], info)`` (``sit_dpc_graph``): what ``pydpc.Cluster(Y,
        fraction)`` computes for the points ``Y`` ``[N, d]``, by the definitions of ``csrc/dpc_plan.h``.  ``info``: the kernel
        milliseconds and the number of pairs."""
        Y = _f64(Y)
        assert Y.ndim == 2
        N, d = Y.shape
        ks = C.c_double(0.0)
        density, delta, nbr, info = np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int32), np.zeros(2)
        self._check(self.lib.sit_dpc_graph(self._h, _d(Y), N, d, float(fraction), C.byref(ks), _d(density), _d(delta),
                                           nbr.ctypes.data_as(_i32p), _d(info)))
        return ks.value, density, delta, nbr, {"kernel_ms": float(info[0]), "pairs": int(info[1])}

    def dpc_assign(self, density, delta, neighbour, min_density, min_delta, dvecs_to_site=None, K=0):
        """``(membership int32 [N], clusters int32 [n_clusters], votes int64 [K, n_clusters] or None)`` (``sit_dpc_assign``):
        centres are the points with ``density > min_density`` and ``delta > min_delta``, every other point follows its neighbour;
        ``votes[s, m]`` counts the points of site ``dvecs_to_site[i] == s`` with membership ``m``."""
        density, delta = _f64(density).reshape(-1), _f64(delta).reshape(-1)
        neighbour = np.ascontiguousarray(neighbour, dtype=np.int32).reshape(-1)
        N = len(density)
        assert len(delta) == N == len(neighbour)
        K = int(K) if dvecs_to_site is not None else 0
        site = _i64(dvecs_to_site).reshape(-1) if dvecs_to_site is not None else None
        assert site is None or len(site) == N
        membership, clusters = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
        nc = i64(0)
        guess = int(np.count_nonzero((density > min_density) & (delta > min_delta)))
        votes = np.zeros((K, guess), dtype=np.int64) if K > 0 else None
        self._check(self.lib.sit_dpc_assign(self._h, _d(density), _d(delta), neighbour.ctypes.data_as(_i32p), N, float(min_density),
                                            float(min_delta), None if site is None else _i(site), K,
                                            membership.ctypes.data_as(_i32p), clusters.ctypes.data_as(_i32p), C.byref(nc),
                                            None if votes is None else _i(votes), 0 if votes is None else votes.size))
        assert int(nc.value) == guess
        return membership, clusters[:guess].copy(), votes

    # ---- RCCL exchange of the frame-sharded path (csrc/comm.hip) ----
    def comm_create(self, unique_id, rank, world):
        uid = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
        assert uid.size == 128
        self._check(self.lib.sit_comm_create(self._h, uid.ctypes.data_as(_u8p), int(rank), int(world)))

    def comm_destroy(self):
        self.lib.sit_comm_destroy(self._h)

    def comm_info(self):
        """What the RCCL communicator reports about itself (``sit_comm_info``)."""
        v = np.zeros(6, dtype=np.int32)
        self._check(self.lib.sit_comm_info(self._h, v.ctypes.data_as(_i32p)))
        return {"ranks": int(v[0]), "rank": int(v[1]), "device": int(v[2]), "rccl_version": int(v[3]),
                "asked_ranks": int(v[4]), "asked_rank": int(v[5])}

    def comm_allreduce(self, arr, op="sum"):
        """In place on a contiguous float64 / int64 / uint64 array."""
        code = {np.dtype(np.float64): 0, np.dtype(np.int64): 1, np.dtype(np.uint64): 2}[arr.dtype]
        assert arr.flags.c_contiguous
        self._check(self.lib.sit_comm_allreduce(self._h, arr.ctypes.data_as(C.c_void_p), arr.size, code,
                                                {"sum": 0, "min": 1, "max": 2}[op]))
        return arr

    def comm_allgather(self, send, world):
        send = np.ascontiguousarray(send)
        recv = np.empty((world,) + send.shape, dtype=send.dtype)
        self._check(self.lib.sit_comm_allgather(self._h, send.ctypes.data_as(C.c_void_p), recv.ctypes.data_as(C.c_void_p),
                                                send.nbytes))
        return recv

    def comm_broadcast(self, arr, root):
        assert arr.flags.c_contiguous
        self._check(self.lib.sit_comm_broadcast(self._h, arr.ctypes.data_as(C.c_void_p), arr.nbytes, int(root)))
        return arr

    def comm_barrier(self):
        self._check(self.lib.sit_comm_barrier(self._h))

    def comm_attach(self, comm_ctx):
        """``gram`` / ``weighted_row_sums`` (and their limbs) of this context return the sums over all ranks of
        ``comm_ctx``'s communicator, reduced on the device (``sit_comm_attach``); ``None`` detaches."""
        self._check(self.lib.sit_comm_attach(self._h, comm_ctx._h if comm_ctx is not None else None))

    def timers(self):
        t = np.zeros(8)
        self.lib.sit_timers(self._h, _d(t), 8)
        return dict(zip(["fill", "fit", "predict", "gram", "site_centers", "occupancy", "h2d"], t))

    def timer_totals(self):
        """(sum of all laps in ms, number of laps) per stage since the context was made."""
        t = np.zeros(24)
        self.lib.sit_timers(self._h, _d(t), 24)
        names = ["fill", "fit", "predict", "gram", "site_centers", "occupancy", "h2d"]
        return {k: (float(t[8 + i]), int(t[16 + i])) for i, k in enumerate(names)}

    def clamp_kernel_time(self):
        """(sum in ms, number) of the ``k_clamp`` launches of ``clamp_trajectory`` since the context was made: the
        kernel alone, without the copies of a call (slot 7 of ``sit_timers``)."""
        t = np.zeros(24)
        self.lib.sit_timers(self._h, _d(t), 24)
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
        head = (self._h, int(which), G.ctypes.data_as(_i32p), C.byref(disp), C.byref(rb), C.byref(total))
        self._check(self.lib.sit_candidate_table(*head, 0, None, 0, None, None))
        nb, n = int(G[0]) * int(G[1]) * int(G[2]), int(total.value)
        off = np.zeros(nb + 1, dtype=np.int32)
        lst = np.zeros(max(n, 1), dtype=np.int32)
        crit = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.lib.sit_candidate_table(*head, nb + 1, off.ctypes.data_as(_i32p), len(lst), lst.ctypes.data_as(_i32p),
                                                 crit.ctypes.data_as(_u8p)))
        return {"grid": [int(x) for x in G], "displacement": disp.value, "rb": rb.value, "total": n, "off": off,
                "list": lst[:n], "crit": crit[:n]}

    def synchronize(self):
        self._check(self.lib.sit_synchronize(self._h))


def _settling(fn):
    """Deferred ``fill`` passes are collected before their output is read: a failed pass raises here (as the reference
    raises from inside its frame loop, landmark/helpers.pyx:76-92,116-118), a pass that outgrew its row buffers is run
    again at the rigorous width (``fill_result``)."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        if self._deferred:
            rc, _, err = self.fill_result()
            self._check(rc, err)
        return fn(self, *args, **kwargs)
    return wrapper


for _name in ("rows_dense", "rows_sparse", "fit_push_stored_rows", "predict", "assignments", "count_zero_rows", "gram",
              "gram_limbs", "weighted_row_sums", "weighted_row_sums_limbs", "best_match", "best_match_groups",
              "site_anchors", "site_sums", "check_occupancy", "site_counts", "cooccupancy", "jump_sources", "jump_list",
              "jump_analysis", "assign_last_known", "running_mode", "set_centers", "label_ends", "replace_unassigned",
              "unknown_runs", "replace_closer", "clamp_trajectory", "group_by_site", "grouped_fetch", "grouped_bucket_averages",
              "grouped_recenter_step", "grouped_hull_volumes", "grouped_work_fetch", "min_image", "pathway_components",
              "barrier_energies", "voronoi_nodes", "coordination_environments", "soap_vectors", "soap_site_averages", "pca_covariance", "pca_project", "dpc_graph",
              "dpc_assign"):
    setattr(HipContext, _name, _settling(getattr(HipContext, _name)))
del _name
