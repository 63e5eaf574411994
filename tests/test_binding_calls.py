"""CPU-only: every call ``sitator_amd/_lib.py`` makes into the library, against the ctypes table it declares.

The loaded library is replaced by a stub whose ``sit_X`` is built from ``SIGNATURES["sit_X"]``: it checks the arity,
converts every argument with ``argtypes[i].from_param`` (what ctypes itself would do, so a float64 pointer where an int32
pointer is declared fails here and not on the device), records the call and returns a scripted status.  ``CALLS`` drives
every public method of ``HipContext`` at the smallest sizes, with every optional array given and left out.
"""
import ctypes as C

import numpy as np
import pytest

from sitator_amd import _lib, errors
from sitator_amd._lib import HipContext, SIGNATURES

F, M, K, D, S, A = 5, 2, 3, 3, 4, 6


def _byref_set(pos, *values):
    def effect(args):
        for p, v in zip(range(pos, pos + len(values)), values):
            args[p]._obj.value = v
    return effect


def _pointer_set(pos, ctype, values):
    def effect(args):
        p = C.cast(args[pos], C.POINTER(ctype))
        for k, v in values.items():
            p[k] = v
    return effect


def _both(*effects):
    def effect(args):
        for e in effects:
            e(args)
    return effect


# what the library writes back where a method goes on to read it
EFFECTS = {
    "sit_create": _byref_set(3, 0x2000),
    "sit_row_width": _byref_set(1, 2),
    "sit_fit_get_state": _byref_set(3, 2),
    "sit_voronoi_nodes": _byref_set(6, 2, 3),
    "sit_coordination_environments": _byref_set(10, 3),
    "sit_soap_site_averages": _byref_set(25, 2),
    "sit_candidate_table": _both(_pointer_set(2, C.c_int32, {0: 1, 1: 2, 2: 1}), _byref_set(5, 3)),
    "sit_dpc_assign": _byref_set(11, 1),
    "sit_group_info": _pointer_set(1, C.c_double, {0: 4.0, 1: float(K)}),
    "sit_coordenv_plan": _both(_pointer_set(0, C.c_int64, {7: len(_lib.COORDENV_SHAPES)}),
                               _pointer_set(1, C.c_int32, {s: 1 for s in range(len(_lib.COORDENV_SHAPES))})),
}


class Stub(object):
    def __init__(self):
        self.calls = []                 # (symbol, args)
        self.rc = {}                    # symbol -> status, or a list of them used up in order
        self.message = b""
        self.effects = dict(EFFECTS)

    def names(self):
        return [c[0] for c in self.calls]

    def of(self, name):
        return [c[1] for c in self.calls if c[0] == name]

    def __getattr__(self, name):
        if name not in SIGNATURES:
            raise AttributeError(name)
        res, argtypes = SIGNATURES[name]

        def call(*args):
            assert len(args) == len(argtypes), "%s: %d arguments, %d declared" % (name, len(args), len(argtypes))
            for k, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as e:
                    raise AssertionError("%s: argument %d (%r) is no %s: %s" % (name, k, a, t.__name__, e))
            self.calls.append((name, args))
            if name in self.effects:
                self.effects[name](args)
            if name == "sit_last_message":
                return self.message
            if res is None:
                return None
            rc = self.rc.get(name, 0)
            return rc.pop(0) if isinstance(rc, list) else rc
        return call


def make_ctx(stub):
    ctx = object.__new__(HipContext)
    ctx.lib = stub
    ctx._h = C.c_void_p(0x1000)
    ctx.device = 0
    ctx.cell = np.eye(3) * 10.0
    ctx.cell_centroid = np.full(3, 5.0)
    ctx.D, ctx.S, ctx.M, ctx.F, ctx.K, ctx.A, ctx.V = D, S, M, F, K, A, 2
    ctx.N = F * M
    ctx.frame0 = 0
    ctx.labels_version = 0
    ctx.labels_digest = None
    ctx._deferred = 0
    ctx._last_fill = None
    return ctx


@pytest.fixture
def stub():
    return Stub()


@pytest.fixture
def ctx(stub):
    c = make_ctx(stub)
    yield c
    c._h = None


def f(*shape):
    return (np.arange(int(np.prod(shape)), dtype=np.float64) / 7.0 + 0.25).reshape(shape)


def n(*shape, **kw):
    return (np.arange(int(np.prod(shape)), dtype=np.int64) % kw.get("mod", K)).reshape(shape)


def soap():
    return {"alpha": f(2, 2), "beta": f(2, 2, 2), "l_max": 1, "n_max": 2, "cutoff": 3.0, "cutoff_transition_width": 0.5,
            "atom_sigma": 0.4, "n_species": 1, "crossover": True, "n_dim": 3}


ROLE = [-1, -1, -1, -1, 0, 1]
STATIC, MOBILE = [0, 1, 2, 3], [4, 5]


def _predict_prefaulted(c):
    c.prefault_assignments(c.N)
    return c.predict(0.5)


def _attach_other(c):
    other = make_ctx(c.lib)
    try:
        c.comm_attach(other)
    finally:
        other._h = None


# every public method of HipContext: its calls, the first the plain one, the others with the optional branches turned
CALLS = {
    "close": [lambda c: c.close()],
    "message": [lambda c: c.message()],
    "wrap_points": [lambda c: c.wrap_points(f(2, 3))],
    "distances": [lambda c: c.distances(f(3), f(2, 3))],
    "average": [lambda c: c.average(f(2, 3)), lambda c: c.average(f(2, 3), f(2))],
    "min_image": [lambda c: c.min_image(f(2, 3), f(2, 3))],
    "site_vertex_distances": [lambda c: c.site_vertex_distances(f(K, 3), f(S, 3), n(K, 2, mod=S))],
    "set_basis": [lambda c: c.set_basis(f(S, 3), n(D, 2, mod=S), f(D, 2), 1.0, 2.0, 0.5)],
    "frames_device_ptr": [lambda c: c.frames_device_ptr()],
    "set_frames": [lambda c: c.set_frames(f(F, A, 3), STATIC, MOBILE, frame0=7)],
    "upload_fill_fit": [lambda c: c.upload_fill_fit(f(F, A, 3), STATIC, MOBILE, 0, False, False, True, 0.9)],
    "row_width": [lambda c: c.row_width()],
    "fill": [lambda c: c.fill(), lambda c: c.fill(assign=True, predict_threshold=0.5, defer=True)],
    "fill_result": [lambda c: c.fill_result()],
    "static_seen": [lambda c: c.static_seen(1)],
    "rows_dense": [lambda c: c.rows_dense(), lambda c: c.rows_dense(2, 3)],
    "rows_sparse": [lambda c: c.rows_sparse(), lambda c: c.rows_sparse(2, 3)],
    "set_rows_dense": [lambda c: c.set_rows_dense(f(4, D))],
    "fit_reset": [lambda c: c.fit_reset()],
    "fit_set_state": [lambda c: c.fit_set_state(f(2, D), [1, 2])],
    "fit_get_state": [lambda c: c.fit_get_state()],
    "fit_push_stored_rows": [lambda c: c.fit_push_stored_rows(0.9)],
    "fit_push_dense_rows": [lambda c: c.fit_push_dense_rows(f(2, D), [1, 1], 0.9)],
    "set_centers": [lambda c: c.set_centers(f(K, D), True)],
    "prefault_assignments": [lambda c: c.prefault_assignments(c.N)],
    "predict": [lambda c: c.predict(0.5), lambda c: c.predict(0.5, fetch=False), _predict_prefaulted],
    "assignments": [lambda c: c.assignments()],
    "count_zero_rows": [lambda c: c.count_zero_rows()],
    "gram": [lambda c: c.gram()],
    "gram_limbs": [lambda c: c.gram_limbs()],
    "weighted_row_sums_limbs": [lambda c: c.weighted_row_sums_limbs(K), lambda c: c.weighted_row_sums_limbs(K, False)],
    "best_match": [lambda c: c.best_match(f(D))],
    "best_match_groups": [lambda c: c.best_match_groups(n(D, mod=2), f(D), 2)],
    "weighted_row_sums": [lambda c: c.weighted_row_sums(K)],
    "site_anchors": [lambda c: c.site_anchors(K, True)],
    "site_sums": [lambda c: c.site_sums(K, True, f(K, 3))],
    "check_occupancy": [lambda c: c.check_occupancy(K, 1)],
    "set_assignments": [lambda c: c.set_assignments(n(F, M)), lambda c: c.set_assignments(n(F, M), f(F, M), frame0=3)],
    "site_counts": [lambda c: c.site_counts(K)],
    "cooccupancy": [lambda c: c.cooccupancy(K)],
    "jump_sources": [lambda c: c.jump_sources(), lambda c: c.jump_sources(True, n(M))],
    "jump_list": [lambda c: c.jump_list(), lambda c: c.jump_list(True, n(M))],
    "jump_analysis": [lambda c: c.jump_analysis(K), lambda c: c.jump_analysis(K, n(M), n(M))],
    "assign_last_known": [lambda c: c.assign_last_known(2),
                          lambda c: c.assign_last_known(2, n(M), n(M), out=np.zeros((F, M), dtype=np.int64))],
    "label_ends": [lambda c: c.label_ends()],
    "replace_unassigned": [lambda c: c.replace_unassigned(0), lambda c: c.replace_unassigned(1, n(M), n(M))],
    "unknown_runs": [lambda c: c.unknown_runs(), lambda c: c.unknown_runs(n(M), n(M))],
    "replace_closer": [lambda c: c.replace_closer(n(1, 6), f(K, 3), f(2, 3))],
    "running_mode": [lambda c: c.running_mode(1, 1, 2, True), lambda c: c.running_mode(1, 1, 2, False, n_sites=K)],
    "recenter": [lambda c: c.recenter(f(F, A, 3), f(A), f(A)), lambda c: c.recenter(f(F, A, 3), f(A), f(A), add3=f(3))],
    "recenter_resident": [lambda c: c.recenter_resident(f(A), f(A)), lambda c: c.recenter_resident(f(A), f(A), add3=f(3))],
    "speed_spectrum": [lambda c: c.speed_spectrum(f(3), [1, 0, 1], positions=f(F, 2, 3)),
                       lambda c: c.speed_spectrum(f(3), [1, 0, 1], atoms=MOBILE, workspace_bytes=1024, spectrum=True, speeds=True)],
    "msd": [lambda c: c.msd(positions=f(F, 2, 3)),
            lambda c: c.msd(atoms=MOBILE, unwrap=False, lags=[1, 2], collective=True, r4=True, images=True)],
    "clamp_trajectory": [lambda c: c.clamp_trajectory(ROLE, f(A, 3), f(K, 3), True, False),
                         lambda c: c.clamp_trajectory(ROLE, f(A, 3), f(K, 3), False, True, positions=f(F, A, 3), workspace_bytes=64)],
    "group_by_site": [lambda c: c.group_by_site(K), lambda c: c.group_by_site(K, positions=f(4, A, 3), mobile_idx=MOBILE)],
    "grouped_fetch": [lambda c: c.grouped_fetch(0, 2), lambda c: c.grouped_fetch(1, 2, points=False, confidences=True, entries=True)],
    "grouped_bucket_averages": [lambda c: c.grouped_bucket_averages(K, 2, True)],
    "grouped_recenter_step": [lambda c: c.grouped_recenter_step(0, 2, None),
                              lambda c: c.grouped_recenter_step(1, 2, np.zeros((4, 3)))],
    "grouped_hull_volumes": [lambda c: c.grouped_hull_volumes(K), lambda c: c.grouped_hull_volumes(K, vertex_mask=True)],
    "grouped_work_fetch": [lambda c: c.grouped_work_fetch(0, 2)],
    "group_info": [lambda c: c.group_info()],
    "pathway_components": [lambda c: c.pathway_components(n(K, K, mod=2), f(K, 3)),
                           lambda c: c.pathway_components(n(K, K, mod=2), f(K, 3), n_images=1, codes=True)],
    "barrier_energies": [lambda c: c.barrier_energies(f(S, 3), f(S), f(S), 3.0, f(K, 3), [[0, 1], [1, 2]], f(3), 0.5),
                         lambda c: c.barrier_energies(f(S, 3), f(S), f(S), 3.0, f(K, 3), [[0, 1]], f(3), 0.5, energies=False,
                                                      codes=True)],
    "voronoi_nodes": [lambda c: c.voronoi_nodes(f(S, 3), 1e-6)],
    "coordination_environments": [lambda c: c.coordination_environments(f(S, 3), f(K, 3))],
    "soap_vectors": [lambda c: c.soap_vectors(f(S, 3), [0] * S, f(K, 3), soap()),
                     lambda c: c.soap_vectors(f(S, 3), [0] * S, f(K, 3), soap(), nbr_count=True)],
    "soap_site_averages": [lambda c: c.soap_site_averages(K, STATIC, [0] * S, MOBILE, soap()),
                           lambda c: c.soap_site_averages(K, STATIC, [0] * S, MOBILE, soap(), stepsize=2, averaging=2,
                                                          avg_descriptors_per_site=1, positions=f(4, A, 3), workspace_bytes=64)],
    "pca_covariance": [lambda c: c.pca_covariance(f(4, D))],
    "pca_project": [lambda c: c.pca_project(f(4, D), f(D), f(2, D))],
    "dpc_graph": [lambda c: c.dpc_graph(f(4, 2))],
    "dpc_assign": [lambda c: c.dpc_assign([1.0, 0, 0, 0], [1.0, 0, 0, 0], [0, 0, 0, 0], 0.5, 0.5),
                   lambda c: c.dpc_assign([1.0, 0, 0, 0], [1.0, 0, 0, 0], [0, 0, 0, 0], 0.5, 0.5, dvecs_to_site=n(4), K=K)],
    "comm_create": [lambda c: c.comm_create(bytes(128), 0, 1)],
    "comm_destroy": [lambda c: c.comm_destroy()],
    "comm_info": [lambda c: c.comm_info()],
    "comm_allreduce": [lambda c: c.comm_allreduce(f(3)), lambda c: c.comm_allreduce(n(3), op="max"),
                       lambda c: c.comm_allreduce(np.zeros(3, dtype=np.uint64), op="min")],
    "comm_allgather": [lambda c: c.comm_allgather(f(3), 2)],
    "comm_broadcast": [lambda c: c.comm_broadcast(n(3), 0)],
    "comm_barrier": [lambda c: c.comm_barrier()],
    "comm_attach": [lambda c: c.comm_attach(None), _attach_other],
    "timers": [lambda c: c.timers()],
    "timer_totals": [lambda c: c.timer_totals()],
    "clamp_kernel_time": [lambda c: c.clamp_kernel_time()],
    "info": [lambda c: c.info()],
    "candidate_table": [lambda c: c.candidate_table(0)],
    "synchronize": [lambda c: c.synchronize()],
}

# the functions of the module that reach the library through load()
MODULE_CALLS = [
    lambda: _lib.device_count(),
    lambda: _lib.comm_unique_id(),
    lambda: _lib.release_cached_memory(),
    lambda: _lib.group_plan(10, K),
    lambda: _lib.hull_plan(),
    lambda: _lib.barrier_plan(np.eye(3) * 10.0, 3.0),
    lambda: _lib.soap_plan(np.eye(3) * 10.0, 3.0, 1, 2, 1),
    lambda: _lib.dpc_plan(2),
    lambda: _lib.voronoi_plan(np.eye(3) * 10.0, S),
    lambda: _lib.coordenv_plan(),
    lambda: HipContext(np.eye(3) * 10.0, device=0).close(),
]

# the methods that collect deferred fill passes before they run
SETTLING = {"rows_dense", "rows_sparse", "fit_push_stored_rows", "predict", "assignments", "count_zero_rows", "gram",
            "gram_limbs", "weighted_row_sums", "weighted_row_sums_limbs", "best_match", "best_match_groups",
            "site_anchors", "site_sums", "check_occupancy", "site_counts", "cooccupancy", "jump_sources", "jump_list",
            "jump_analysis", "assign_last_known", "running_mode", "set_centers", "label_ends", "replace_unassigned",
            "unknown_runs", "replace_closer", "clamp_trajectory", "group_by_site", "grouped_fetch", "grouped_bucket_averages",
            "grouped_recenter_step", "grouped_hull_volumes", "grouped_work_fetch", "min_image", "pathway_components",
            "barrier_energies", "voronoi_nodes", "coordination_environments", "soap_vectors", "soap_site_averages",
            "pca_covariance", "pca_project", "dpc_graph", "dpc_assign"}

# (symbol, argument) of every pointer a method may leave out
OPTIONAL = {("sit_average", 2), ("sit_fit_get_state", 1), ("sit_fit_get_state", 2), ("sit_predict", 2), ("sit_predict", 3),
            ("sit_set_assignments", 2), ("sit_jump_sources", 2), ("sit_jump_list", 2), ("sit_jump_analysis", 2),
            ("sit_jump_analysis", 3), ("sit_assign_last_known", 2), ("sit_assign_last_known", 3), ("sit_replace_unassigned", 2),
            ("sit_replace_unassigned", 3), ("sit_unknown_runs", 1), ("sit_unknown_runs", 2), ("sit_running_mode", 7),
            ("sit_recenter", 6), ("sit_recenter_resident", 3), ("sit_speed_spectrum", 1), ("sit_speed_spectrum", 3),
            ("sit_speed_spectrum", 10), ("sit_speed_spectrum", 11), ("sit_msd", 1), ("sit_msd", 3), ("sit_msd", 7), ("sit_msd", 12),
            ("sit_msd", 13), ("sit_msd", 14), ("sit_clamp_trajectory", 1), ("sit_group_by_site", 1), ("sit_group_by_site", 4),
            ("sit_grouped_fetch", 3), ("sit_grouped_fetch", 4), ("sit_grouped_fetch", 5), ("sit_grouped_recenter_step", 3),
            ("sit_grouped_hull_volumes", 4), ("sit_pathway_components", 5), ("sit_barrier_energies", 13),
            ("sit_barrier_energies", 15), ("sit_voronoi_nodes", 8), ("sit_voronoi_nodes", 9), ("sit_voronoi_nodes", 10),
            ("sit_voronoi_nodes", 11), ("sit_coordination_environments", 14), ("sit_coordination_environments", 15),
            ("sit_coordination_environments", 16), ("sit_coordination_environments", 17), ("sit_soap_vectors", 17),
            ("sit_soap_site_averages", 1), ("sit_soap_site_averages", 28), ("sit_dpc_assign", 7), ("sit_dpc_assign", 12),
            ("sit_candidate_table", 7), ("sit_candidate_table", 9), ("sit_candidate_table", 10), ("sit_comm_attach", 1)}


def run_all(stub):
    """Every call of ``CALLS`` on a fresh context each, then ``MODULE_CALLS`` with ``load()`` giving the stub."""
    for name in CALLS:
        for call in CALLS[name]:
            c = make_ctx(stub)
            try:
                call(c)
            finally:
                c._h = None
    saved = _lib._lib
    _lib._lib = stub
    try:
        for call in MODULE_CALLS:
            call()
    finally:
        _lib._lib = saved


def public_methods():
    return {k for k, v in vars(HipContext).items() if callable(v) and not k.startswith("_")}


# ---- coverage
def test_calls_cover_every_public_method():
    assert set(CALLS) == public_methods()
    assert SETTLING <= set(CALLS) and len(SETTLING) == 45


def test_every_symbol_is_reached_with_the_declared_arguments(stub):
    run_all(stub)
    # sit_abi belongs to load() itself; sit_set_frames_device is declared for callers that hold a device pointer and
    # has no method of HipContext
    assert set(stub.names()) == set(SIGNATURES) - {"sit_abi", "sit_set_frames_device"}


def test_every_optional_pointer_is_given_and_left_out(stub):
    run_all(stub)
    none, given = set(), set()
    for name, args in stub.calls:
        for k, (t, a) in enumerate(zip(SIGNATURES[name][1], args)):
            if k > 0 and (t is _lib._vp or hasattr(t, "contents")):
                (none if a is None else given).add((name, k))
    assert none == OPTIONAL
    assert OPTIONAL <= given


# ---- status mapping
def test_check_maps_the_status_codes(stub, ctx):
    stub.message = b"no such thing"
    for rc, exc in ((_lib.E_INVALID, ValueError), (_lib.E_NOT_CONVERGED, ValueError)):
        stub.rc["sit_synchronize"] = rc
        with pytest.raises(exc, match="no such thing") as e:
            ctx.synchronize()
        assert not isinstance(e.value, IndexError)
    for rc in (_lib.E_HIP, _lib.E_CAPACITY):
        stub.rc["sit_synchronize"] = rc
        with pytest.raises(RuntimeError, match="libsitator_hip: no such thing"):
            ctx.synchronize()
    stub.rc["sit_synchronize"] = _lib.RETRY
    with pytest.raises(RuntimeError, match="SIT_RETRY"):
        ctx.synchronize()
    stub.rc["sit_synchronize"] = _lib.E_ZERO_LANDMARK
    with pytest.raises(errors.DeviceDomainError) as e:
        ctx.synchronize()
    assert (e.value.kind, e.value.frame, e.value.index) == (_lib.E_ZERO_LANDMARK, -1, -1)
    stub.rc["sit_synchronize"] = _lib.OK
    ctx.synchronize()


INDEXED = ["cooccupancy", "jump_analysis", "replace_closer", "clamp_trajectory", "group_by_site", "grouped_recenter_step",
           "soap_site_averages"]


@pytest.mark.parametrize("name", INDEXED)
def test_index_messages_become_index_errors(stub, ctx, name):
    symbol = {"grouped_recenter_step": "sit_grouped_recenter_step"}.get(name, "sit_" + name)
    stub.rc[symbol] = _lib.E_INVALID
    stub.message = b"index 7 is beyond the 3 sites"
    with pytest.raises(IndexError, match="index 7"):
        CALLS[name][0](ctx)
    stub.message = b"K must be positive"
    with pytest.raises(ValueError, match="K must be positive") as e:
        CALLS[name][0](ctx)
    assert not isinstance(e.value, IndexError)


def test_other_methods_keep_value_error_for_index_messages(stub, ctx):
    stub.rc["sit_site_counts"] = _lib.E_INVALID
    stub.message = b"index 7 is beyond the 3 sites"
    with pytest.raises(ValueError) as e:
        ctx.site_counts(K)
    assert not isinstance(e.value, IndexError)


def test_unassigned_clamp_carries_the_first_entry(stub, ctx):
    stub.rc["sit_clamp_trajectory"] = _lib.E_UNASSIGNED
    stub.effects["sit_clamp_trajectory"] = _byref_set(12, 7)
    with pytest.raises(errors.UnassignedClampError) as e:
        CALLS["clamp_trajectory"][0](ctx)
    assert e.value.first_unassigned == 7


def test_failed_create_raises_and_destroys(stub, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", stub)
    stub.rc["sit_create"] = _lib.E_HIP
    stub.message = b"no device"
    with pytest.raises(RuntimeError, match="sit_create failed on device 0: no device"):
        HipContext(np.eye(3), device=0)
    assert stub.names() == ["sit_create", "sit_last_message", "sit_destroy"]


def test_plan_functions_keep_their_exceptions(stub, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", stub)
    cell = np.eye(3) * 10.0
    plans = {"sit_group_plan": lambda: _lib.group_plan(10, K), "sit_barrier_plan": lambda: _lib.barrier_plan(cell, 3.0),
             "sit_soap_plan": lambda: _lib.soap_plan(cell, 3.0, 1, 2, 1), "sit_dpc_plan": lambda: _lib.dpc_plan(2),
             "sit_voronoi_plan": lambda: _lib.voronoi_plan(cell, S), "sit_coordenv_plan": lambda: _lib.coordenv_plan()}
    for symbol, call in plans.items():
        stub.rc = {symbol: _lib.E_INVALID}
        with pytest.raises(ValueError, match=symbol[4:]):
            call()
    for symbol in ("sit_soap_plan", "sit_dpc_plan"):
        stub.rc = {symbol: _lib.E_CAPACITY}
        with pytest.raises(RuntimeError, match=symbol[4:]):
            plans[symbol]()
    stub.rc = {"sit_comm_unique_id": 1}
    with pytest.raises(RuntimeError, match="sit_comm_unique_id failed"):
        _lib.comm_unique_id()
    stub.rc = {}
    stub.effects["sit_dpc_plan"] = _pointer_set(1, C.c_int64, {0: 256, 4: 8, 11: 99})
    plan = _lib.dpc_plan(2)
    assert (plan["threads"], plan["max_d"], plan["pca_max_n"], len(plan)) == (256, 8, 99, 12)
    stub.effects["sit_soap_plan"] = _pointer_set(5, C.c_int64, {0: 1, 1: 2, 2: 3, 3: 64, 6: 9, 11: 5})
    plan = _lib.soap_plan(cell, 3.0, 1, 2, 1)
    assert (plan["translations"], plan["threads"], plan["max_l"], plan["n_dim_crossover"], len(plan)) == ((1, 2, 3), 64, 9, 5, 10)
    stub.effects["sit_voronoi_plan"] = _both(_pointer_set(2, C.c_int64, {0: 40, 7: 3}), _pointer_set(3, C.c_double, {0: 2.5, 1: 1.5}))
    plan = _lib.voronoi_plan(cell, S)
    assert (plan["neighbour_cap"], plan["inverse_shape_min"], plan["first_radius"], plan["growth"], len(plan)) == (40, 3, 2.5, 1.5, 10)
    stub.effects["sit_barrier_plan"] = _pointer_set(2, C.c_int64, {0: 1, 1: 2, 2: 3, 3: 32, 4: 256, 5: 4096})
    assert _lib.barrier_plan(cell, 3.0) == {"translations": (1, 2, 3), "tile": 32, "threads": 256, "lds_bytes": 4096}
    stub.effects["sit_group_plan"] = _pointer_set(2, C.c_int64, {0: 100, 1: 2, 2: 1, 3: 64})
    assert _lib.group_plan(10, K) == (100, 2, True, 64)
    stub.effects["sit_hull_plan"] = _pointer_set(0, C.c_int64, {0: 5, 1: 6, 2: 7, 3: 8})
    assert _lib.hull_plan() == (5, 6, 7, 8)


def test_timer_block_is_read_by_slot(stub, ctx):
    stub.effects["sit_timers"] = lambda args: _pointer_set(1, C.c_double, {k: float(k) for k in range(args[2])})(args)
    stages = ["fill", "fit", "predict", "gram", "site_centers", "occupancy", "h2d"]
    assert ctx.timers() == {k: float(i) for i, k in enumerate(stages)}
    assert ctx.timer_totals() == {k: (8.0 + i, 16 + i) for i, k in enumerate(stages)}
    assert ctx.clamp_kernel_time() == (15.0, 23)
    assert [a[2] for a in stub.of("sit_timers")] == [8, 24, 24]


# ---- deferred passes
# fill_result is the collector itself, and upload_fill_fit starts over
@pytest.mark.parametrize("name", sorted(set(CALLS) - {"fill_result", "upload_fill_fit"}))
def test_deferred_passes_are_collected_by_the_listed_methods_only(stub, ctx, name):
    ctx._deferred = 1
    CALLS[name][0](ctx)
    names = stub.names()
    if name in SETTLING:
        assert names[0] == "sit_fill_result" and names.count("sit_fill_result") == 1 and len(names) > 1
        assert ctx._deferred == 0
    else:
        assert "sit_fill_result" not in names


@pytest.mark.parametrize("name", sorted(SETTLING))
def test_a_failed_deferred_pass_raises_before_the_method_runs(stub, ctx, name):
    def failing(args):
        args[2]._obj.frame, args[2]._obj.index = 3, 1
    stub.rc["sit_fill_result"] = _lib.E_ZERO_LANDMARK
    stub.effects["sit_fill_result"] = failing
    ctx._deferred = 2
    with pytest.raises(errors.DeviceDomainError) as e:
        CALLS[name][0](ctx)
    assert (e.value.kind, e.value.frame, e.value.index) == (_lib.E_ZERO_LANDMARK, 3, 1)
    assert stub.names() == ["sit_fill_result"]


def test_fill_counts_deferred_passes_and_fill_result_repeats_on_retry(stub, ctx):
    assert ctx.fill(defer=True)[0] == _lib.OK and ctx._deferred == 1
    assert ctx.fill(defer=True)[0] == _lib.OK and ctx._deferred == 2
    assert stub.of("sit_fill")[-1][1]._obj.defer == 1
    stub.rc["sit_fill_result"] = _lib.RETRY
    stub.effects["sit_fill"] = _byref_set(2, 4)
    rc, nz, err = ctx.fill_result()
    assert (rc, nz, ctx._deferred) == (_lib.OK, 4, 0)
    assert stub.names() == ["sit_fill", "sit_fill", "sit_fill_result", "sit_fill"]
    assert stub.calls[-1][1][1]._obj.defer == 0
    stub.rc["sit_fill"] = _lib.E_HIP
    assert ctx.fill(defer=True)[0] == _lib.E_HIP and ctx._deferred == 0


# ---- label mark
WRITERS = {("fill", 1), ("predict", 0), ("predict", 1), ("predict", 2), ("set_assignments", 0), ("set_assignments", 1),
           ("assign_last_known", 0), ("assign_last_known", 1)}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_only_the_label_writers_mark_the_labels_rewritten(stub, name):
    for k, call in enumerate(CALLS[name]):
        c = make_ctx(stub)
        c.labels_version, c.labels_digest = 5, (5, "digest")
        try:
            call(c)
            if (name, k) in WRITERS:
                assert (c.labels_version, c.labels_digest) == (6, None), (name, k)
            else:
                assert (c.labels_version, c.labels_digest) == (5, (5, "digest")), (name, k)
        finally:
            c._h = None
    assert {w[0] for w in WRITERS} == {"fill", "predict", "set_assignments", "assign_last_known"}


# ---- record loop
@pytest.mark.parametrize("name, symbol, cap_at, rec_at, n_at, width", [("jump_list", "sit_jump_list", 3, 4, 5, 4),
                                                                      ("unknown_runs", "sit_unknown_runs", 3, 4, 5, 6)])
def test_record_loop_repeats_once_with_the_reported_size(stub, ctx, name, symbol, cap_at, rec_at, n_at, width):
    def report(args):
        args[n_at]._obj.value = 70000
        if symbol == "sit_unknown_runs":
            args[6]._obj.value = 123
    stub.effects[symbol] = report
    out = CALLS[name][0](ctx)
    calls = stub.of(symbol)
    assert [a[cap_at] for a in calls] == [1 << 16, 70000]
    assert [a[rec_at]._arr.shape for a in calls] == [(1 << 16, width), (70000, width)]
    assert out[0].shape == (70000, width)
    if name == "unknown_runs":
        assert out[1] == 123
    else:
        rec = out[0]                    # by frame, then by atom
        assert np.all((rec[1:, 0] > rec[:-1, 0]) | ((rec[1:, 0] == rec[:-1, 0]) & (rec[1:, 1] >= rec[:-1, 1])))


def test_record_loop_does_not_repeat_when_the_records_fit(stub, ctx):
    stub.effects["sit_jump_list"] = _byref_set(5, 1 << 16)
    assert ctx.jump_list()[0].shape == (1 << 16, 4)
    stub.effects["sit_unknown_runs"] = _byref_set(5, 3)
    assert ctx.unknown_runs()[0].shape == (3, 6)
    assert stub.names() == ["sit_jump_list", "sit_unknown_runs"]


# ---- two-call protocols: the second call's capacities are the sizes the first reported
def test_two_call_protocols(stub, ctx):
    centers, counts = ctx.fit_get_state()
    first, second = stub.of("sit_fit_get_state")
    assert first[1] is None and first[2] is None
    assert second[1]._arr is centers and second[2]._arr is counts and centers.shape == (2, D) and counts.shape == (2,)

    res = ctx.voronoi_nodes(f(S, 3), 1e-6)
    first, second = stub.of("sit_voronoi_nodes")
    assert (first[4], first[5], second[4], second[5]) == (0, 0, 2, 3)
    assert second[8]._arr.shape == (2, 3) and second[9]._arr.shape == (2,) and second[10]._arr.shape == (3,) and second[11]._arr.shape == (3,)
    assert res["centers"].shape == (2, 3) and len(res["vertices"]) == 2

    res = ctx.coordination_environments(f(S, 3), f(K, 3))
    first, second = stub.of("sit_coordination_environments")
    assert (first[9], second[9]) == (0, 3)
    assert second[14]._arr.shape == (K + 1,) and [second[k]._arr.shape for k in (15, 16, 17)] == [(3,)] * 3

    descs = ctx.soap_site_averages(K, STATIC, [0] * S, MOBILE, soap())[0]
    first, second = stub.of("sit_soap_site_averages")
    assert (first[24], first[28], second[24]) == (0, None, 2)
    assert second[28]._arr is descs and descs.shape == (2, 3)

    table = ctx.candidate_table(1)
    first, second = stub.of("sit_candidate_table")
    assert (first[6], first[8], second[6], second[8]) == (0, 0, 3, 3)
    assert second[7]._arr is table["off"] and table["off"].shape == (3,) and table["grid"] == [1, 2, 1] and table["total"] == 3


def test_fit_get_state_of_no_centre_makes_one_call(stub, ctx):
    stub.effects["sit_fit_get_state"] = _byref_set(3, 0)
    centers, counts = ctx.fit_get_state()
    assert centers.shape == (0, D) and counts.shape == (0,) and stub.names() == ["sit_fit_get_state"]


# ---- what the methods assert about their arrays
def test_shape_and_layout_assertions(stub, ctx):
    with pytest.raises(AssertionError):
        ctx.clamp_trajectory(ROLE, f(A, 3), f(K, 3), True, False, positions=f(F, A - 1, 3))
    with pytest.raises(AssertionError):
        ctx.group_by_site(K, positions=f(F, A, 2), mobile_idx=MOBILE)
    with pytest.raises(AssertionError):
        ctx.soap_site_averages(K, STATIC, [0] * S, MOBILE, soap(), positions=f(F, A * 3))
    with pytest.raises(AssertionError):
        ctx.speed_spectrum(f(3), [1, 0, 1], positions=f(F, 2, 2))
    with pytest.raises(AssertionError):
        ctx.recenter(f(F, A, 3).astype(np.float32), f(A), f(A))
    with pytest.raises(AssertionError):
        ctx.grouped_recenter_step(0, 2, f(3, 4).T)
    with pytest.raises(AssertionError):
        ctx.assign_last_known(2, out=np.zeros((F, M), dtype=np.int32))
    with pytest.raises(AssertionError):
        ctx.comm_broadcast(f(3, 4).T, 0)
    with pytest.raises(AssertionError):
        ctx.comm_allreduce(f(3, 4).T)
    with pytest.raises(KeyError):
        ctx.comm_allreduce(np.zeros(3, dtype=np.float32))
    with pytest.raises(ValueError, match="explicit lag list"):
        ctx.msd(positions=f(F, 2, 3), r4=True)
    with pytest.raises(ValueError, match="come as a pair"):
        ctx.unknown_runs(before_in=n(M))
    assert stub.calls == []


# ---- the marshalling guard and the context manager (what the binding refactor adds)
def test_ptr_checks_what_it_hands_over():
    assert _lib._ptr(None) is None and _lib._d(None) is None and _lib._i(None) is None
    table = {np.float64: _lib._dp, np.complex128: _lib._dp, np.int64: _lib._ip, np.int32: _lib._i32p, np.uint8: _lib._u8p,
             np.uint64: _lib._u64p}
    for dtype, T in table.items():
        a = np.zeros((2, 3), dtype=dtype)
        p = _lib._ptr(a)
        assert type(p) is T and p._arr is a and C.cast(p, C.c_void_p).value == a.ctypes.data
    for bad in (np.float32, np.int16, np.bool_, np.uint32):
        with pytest.raises((AssertionError, TypeError)):
            _lib._ptr(np.zeros(3, dtype=bad))
    for a in (f(3, 4).T, f(6)[::2]):
        with pytest.raises(AssertionError):
            _lib._ptr(a)
    assert type(_lib._d(f(3))) is _lib._dp and type(_lib._i(n(3))) is _lib._ip
    with pytest.raises((AssertionError, TypeError)):
        _lib._d(n(3))
    with pytest.raises((AssertionError, TypeError)):
        _lib._i(f(3))
    with pytest.raises((AssertionError, TypeError)):
        _lib._d(np.zeros(3, dtype=np.complex128))


def test_with_closes_once(stub):
    c = make_ctx(stub)
    with c as inside:
        assert inside is c
        c.synchronize()
    assert stub.names() == ["sit_synchronize", "sit_destroy"] and c._h is None
    c.close()
    assert stub.names().count("sit_destroy") == 1
    c = make_ctx(stub)
    with pytest.raises(ValueError):
        with c:
            stub.rc["sit_synchronize"] = _lib.E_INVALID
            c.synchronize()
    assert stub.names().count("sit_destroy") == 2 and c._h is None
